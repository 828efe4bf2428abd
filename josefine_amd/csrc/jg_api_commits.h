// jg_api_commits.h - jg_engine_watch_commits: the commit feed (jg_commits.h).  A call that reads, under the rules of
// jg_api_manage.h and in the shape of jg_api_isr.h: refused while kept node steps are outstanding, JG_NODE_ASYNC steps
// settled, the scratch carved from the engine's staging, a multi-device handle served shard by shard.  A call queues its
// passes back to back and synchronises once.  Part of josefine_gpu.hip's one translation unit.
#pragma once

namespace {

// one single-device engine's part of a commit watch: shard-local slots [g0, g0 + n), the first `cap` changed rows
// (groups + add) into host `out`, their shadow advanced unless peeking; *total the slots that differ; w (if not null)
// [JG_CMT_WORDS] the backlog of the range before the delivery
int commit_shard(jg_engine* e, uint32_t flags, uint32_t g0, uint32_t n, uint32_t add, jg_commit_row* out, size_t cap, size_t* total,
                 uint64_t* w) {
  *total = 0;
  if (w) std::memset(w, 0, JG_CMT_WORDS * 8);
  if (!n) return JG_OK;
  HIPCHK(hipSetDevice(e->device));
  {
    const int rc = node_settle(e);
    if (rc) return rc;
  }
  if (!e->commit_shadow) {  // (zero-filled on the engine's stream: every slot was last delivered at genesis)
    const int rc = dev_alloc(e, &e->commit_shadow, e->cfg.n_groups);
    if (rc) return rc;
  }
  JgCommitArgs a{};
  a.g0 = g0, a.n = n, a.add = add;
  a.peek = (flags & JG_WATCH_PEEK) ? 1u : 0u, a.commits_only = (flags & JG_WATCH_COMMITS_ONLY) ? 1u : 0u, a.backlog = w ? 1u : 0u;
  a.tiles = (n + JG_CMT_TILE - 1) / JG_CMT_TILE;
  a.parts = std::min<uint32_t>(a.tiles, JG_CMT_PARTS);
  const size_t wcap = std::min<size_t>(cap, n);
  Carve c;
  const size_t o_total = c.sect(8), o_job = c.sect(sizeof(JgScanJob)), o_sum = c.sect(JG_CMT_WORDS * 8),
               o_part = c.sect((size_t)a.parts * JG_CMT_WORDS * 8), o_cnt = c.sect((size_t)a.tiles * 4), o_bsum = c.sect((size_t)a.tiles * 8),
               o_out = c.sect(wcap * sizeof(jg_commit_row));
  char* B = nullptr;
  if (const int rc = c.on_staging(e, B)) return rc;
  a.shadow = e->commit_shadow;
  a.cnt = (uint32_t*)(B + o_cnt);
  a.bsum = (uint64_t*)(B + o_bsum);
  a.part = (uint64_t*)(B + o_part);
  a.sum = (uint64_t*)(B + o_sum);
  a.out = (uint4*)(B + o_out);
  a.cap = wcap;
  const JgScanJob job{a.bsum, a.tiles, 0};
  HIPCHK(hipMemcpyAsync(B + o_job, &job, sizeof job, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_commit_count, dim3(a.parts), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
  hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(JG_BLOCK), 0, e->stream, (const JgScanJob*)(B + o_job), (uint64_t*)(B + o_total));
  e->n_launch += 2;
  if (w) {
    hipLaunchKernelGGL(k_commit_backlog_sum, dim3(1), dim3(JG_BLOCK), 0, e->stream, a);
    e->n_launch++;
  }
  if (wcap) {  // (queued unseen: a quiet engine's workgroups return after their two loads)
    hipLaunchKernelGGL(k_commit_write, dim3(a.tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
    e->n_launch++;
  }
  HIPCHK(hipGetLastError());
  uint64_t tot = 0;
  HIPCHK(hipMemcpyAsync(&tot, B + o_total, 8, hipMemcpyDeviceToHost, e->stream));
  if (w) HIPCHK(hipMemcpyAsync(w, a.sum, JG_CMT_WORDS * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *total = (size_t)tot;
  const size_t k = std::min<size_t>(wcap, tot);
  if (k) HIPCHK(hipMemcpy(out, a.out, k * sizeof(jg_commit_row), hipMemcpyDeviceToHost));
  return JG_OK;
}

}  // namespace

extern "C" {

int jg_engine_watch_commits(jg_engine* e, uint32_t flags, uint32_t g0, uint32_t n, jg_commit_row* out, size_t cap, size_t* total,
                            jg_commit_backlog* backlog) {
  if (!e || !total || (cap && !out)) return fail(JG_EINVAL, "null argument");
  if (flags & ~(uint32_t)(JG_WATCH_PEEK | JG_WATCH_COMMITS_ONLY)) return fail(JG_EINVAL, "jg_engine_watch_commits: unknown flag");
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_watch_commits: slot range out of bounds");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  uint64_t* bw = (uint64_t*)backlog;  // (jg_commit_backlog is the backlog words in order: jg_commits.h)
  if (!e->router) {  // (straight into the caller's array; the backlog only once the call has succeeded)
    uint64_t w[JG_CMT_WORDS];
    size_t tot = 0;
    const int rc = commit_shard(e, flags, g0, n, 0, out, cap, &tot, bw ? w : nullptr);
    if (rc) return rc;
    *total = tot;
    if (bw) std::memcpy(bw, w, sizeof w);
    return JG_OK;
  }
  // a sharded handle: every shard is sized first (a peek that delivers nothing; the backlog is the shards' sum from that
  // pass), then each shard delivers - and advances - what is left of cap behind the shards before it; a shard behind the
  // point where cap ran out is not called again
  const size_t D = shard_count(e);
  std::vector<size_t> tot(D, 0), at(D + 1, 0);
  std::vector<uint64_t> w(D * JG_CMT_WORDS, 0);
  int rc = each_shard(e, [&](size_t d) -> int {
    const ShardPart sp = shard_part(e, d, g0, n);
    return commit_shard(shard_at(e, d), flags | JG_WATCH_PEEK, sp.g0, sp.n, 0, nullptr, 0, &tot[d], bw ? w.data() + d * JG_CMT_WORDS : nullptr);
  });
  if (rc) return rc;
  for (size_t d = 0; d < D; d++) at[d + 1] = at[d] + tot[d];
  if (cap && at[D]) {
    rc = each_shard(e, [&](size_t d) -> int {
      if (!tot[d] || at[d] >= cap) return JG_OK;
      const ShardPart sp = shard_part(e, d, g0, n);
      size_t again = 0;
      return commit_shard(shard_at(e, d), flags, sp.g0, sp.n, e->router->lo[d], out + at[d], cap - at[d], &again, nullptr);
    });
    if (rc) return rc;
  }
  *total = at[D];
  if (bw) {
    for (uint32_t x = 0; x < JG_CMT_WORDS; x++) {
      uint64_t t = 0;
      for (size_t d = 0; d < D; d++) t += w[d * JG_CMT_WORDS + x];
      bw[x] = t;
    }
  }
  return JG_OK;
}

}  // extern "C"
