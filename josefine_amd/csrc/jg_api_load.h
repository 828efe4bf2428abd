// jg_api_load.h - jg_engine_load_chains: an engine opened on the persisted chain trees of a process that restarts
// (Raft::<Follower>::new + Chain::new on the sled directory, follower.rs:68-95, chain.rs:117-137).  The host checks the
// image's shape, uploads it and launches the passes of jg_load.h; the ascending order of the ids is checked on the device,
// ahead of every write.  The refusals, the shards' parts and the step's bookkeeping are jg_api_manage.h's.  Part of
// josefine_gpu.hip's one translation unit.
#pragma once

namespace {

// one single-device engine: groups [g0, g0 + n) of it, `off` rebased (off[0] == 0)
int load_chains_shard(jg_engine* e, uint64_t now_ms, uint32_t g0, uint32_t n, const uint64_t* off, const uint64_t* id,
                      const uint64_t* next, const uint64_t* commit, const uint8_t* has_commit) {
  if (!n) return JG_OK;
  HIPCHK(hipSetDevice(e->device));
  {
    const int rc = node_settle(e);
    if (rc) return rc;
  }
  const uint64_t rows = off[n];
  const uint64_t tiles = std::max<uint64_t>((rows + JG_LOAD_TILE - 1) / JG_LOAD_TILE, 1);
  // one scratch block: 8-byte sections first, then 4-byte, then 1-byte
  Carve c;
  const size_t o_off = c.sect(((size_t)n + 1) * 8), o_id = c.sect(rows * 8), o_next = c.sect(rows * 8), o_commit = c.sect((size_t)n * 8),
               o_bsum = c.sect(tiles * 8), o_total = c.sect(8), o_job = c.sect(sizeof(JgScanJob)), o_sx = c.sect(rows * 4),
               o_err = c.sect(4), o_has = c.sect(n), o_st = c.sect(rows);
  char* B = nullptr;
  if (const int rc = c.alloc(B)) return rc;
  JgLoadArgs a;
  a.n = n;
  a.g0 = g0;
  a.rows = rows;
  a.off = (const uint64_t*)(B + o_off);
  a.id = (const uint64_t*)(B + o_id);
  a.next = (const uint64_t*)(B + o_next);
  a.commit = (const uint64_t*)(B + o_commit);
  a.has_commit = (const uint8_t*)(B + o_has);
  a.st = (uint8_t*)(B + o_st);
  a.sx = (uint32_t*)(B + o_sx);
  a.bsum = (uint64_t*)(B + o_bsum);
  a.total = (uint64_t*)(B + o_total);
  a.err = (uint32_t*)(B + o_err);
  const JgScanJob job{a.bsum, (uint32_t)tiles, 0};
  HIPCHK(hipMemcpyAsync(B + o_off, off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, e->stream));
  if (rows) {
    HIPCHK(hipMemcpyAsync(B + o_id, id, rows * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(B + o_next, next, rows * 8, hipMemcpyHostToDevice, e->stream));
  }
  HIPCHK(hipMemcpyAsync(B + o_commit, commit, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(B + o_has, has_commit, n, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(B + o_job, &job, sizeof job, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemsetAsync(B + o_err, 0, 4, e->stream));
  HIPCHK(hipMemsetAsync(B + o_total, 0, 8, e->stream));
  if (rows) {
    hipLaunchKernelGGL(k_load_flags, dim3((uint32_t)tiles), dim3(JG_BLOCK), 0, e->stream, a);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(JG_BLOCK), 0, e->stream, (const JgScanJob*)(B + o_job), a.total);
    hipLaunchKernelGGL(k_load_scan, dim3((uint32_t)tiles), dim3(JG_BLOCK), 0, e->stream, a);
    hipLaunchKernelGGL(k_load_place, dim3((uint32_t)((rows + JG_BLOCK - 1) / JG_BLOCK)), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
    e->n_launch += 4;
  }
  groups_rewritten(e);  // (no own slot is written: a loaded group keeps its own)
  e->seq++;
  hipLaunchKernelGGL(k_load_groups, dim3((n + JG_BLOCK - 1) / JG_BLOCK), dim3(JG_BLOCK), 0, e->stream, e->dev, a, now_ms, e->seq);
  HIPCHK(hipGetLastError());
  e->n_launch++;
  uint32_t err = 0;
  HIPCHK(hipMemcpyAsync(&err, a.err, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));  // (the pageable sources and the scratch block are done with)
  if (err) return fail(JG_EINVAL, "jg_engine_load_chains: block ids are not strictly ascending within a group (nothing was loaded)");
  return JG_OK;
}

}  // namespace

extern "C" {

int jg_engine_load_chains(jg_engine* e, uint64_t now_ms, const jg_chain_image* img) {
  if (!e || !img) return fail(JG_EINVAL, "null argument");
  const uint32_t g0 = img->g0, n = img->n;
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_load_chains: group range out of bounds");
  if (!n) return JG_OK;
  if (!img->off || !img->commit || !img->has_commit) return fail(JG_EINVAL, "null argument");
  if (img->off[0] != 0) return fail(JG_EINVAL, "jg_engine_load_chains: off[0] != 0");
  for (uint32_t i = 0; i < n; i++)
    if (img->off[i + 1] < img->off[i]) return fail(JG_EINVAL, "jg_engine_load_chains: off is not monotone");
  const uint64_t rows = img->off[n];
  if (rows >= 0xffffffffull) return fail(JG_EINVAL, "jg_engine_load_chains: too many blocks in one call: split the range");
  if (rows && (!img->blk_id || !img->blk_next)) return fail(JG_EINVAL, "null argument");
  if (const int rc = refuse_first(e, rewrite_refuse)) return rc;
  // a sharded handle checks the ascending order on the host as well: one device's refusal must not come after another
  // device has loaded its part.  Then each shard loads its part on its own device.
  if (e->router)
    for (uint32_t i = 0; i < n; i++)
      for (uint64_t k = img->off[i] + 1; k < img->off[i + 1]; k++)
        if (img->blk_id[k] <= img->blk_id[k - 1])
          return fail(JG_EINVAL, "jg_engine_load_chains: block ids are not strictly ascending within a group (nothing was loaded)");
  return write_shards(e, [&](size_t d) -> int {
    const ShardPart p = shard_part(e, d, g0, n);
    const uint64_t* off = img->off + p.at;
    const uint64_t base = off[0];
    std::vector<uint64_t> rebased;  // (a part that does not begin at the image's first row: its offsets from its own)
    if (base) {
      rebased.resize((size_t)p.n + 1);
      for (uint32_t i = 0; i <= p.n; i++) rebased[i] = off[i] - base;
      off = rebased.data();
    }
    return load_chains_shard(shard_at(e, d), now_ms, p.g0, p.n, off, img->blk_id + base, img->blk_next + base, img->commit + p.at,
                             img->has_commit + p.at);
  });
}

}  // extern "C"
