// jg_api_read.h - jg_engine_read_chains: each group's chain tree read back out as the CSR rows of a sled scan, the
// inverse of jg_engine_load_chains (jg_api_load.h).  The host sizes the read with the group passes of jg_read.h, checks
// the caller's capacity, then writes the rows piece by piece through the engine's staging (jg_api_manage.h's
// staged_pieces): the kernel of piece k + 1 runs while piece k travels to the caller.  Part of josefine_gpu.hip's one
// translation unit.
#pragma once

namespace {

// one single-device engine's part of a read: groups [g0, g0 + n) of it; the device scratch lives until the job ends
struct JgReadJob {
  jg_engine* e = nullptr;
  uint32_t g0 = 0, n = 0, at = 0;  // (at: the part's place in the caller's per-group arrays)
  const uint64_t* from = nullptr;
  uint64_t rows = 0, segs = 0;
  JgReadArgs a{};
  JgScanJob jobs[2]{};
  uint64_t totals[2]{};
  uint32_t err = 0;
  Carve scratch;        // per group and per tile
  char* T = nullptr;    // the segment table
  ~JgReadJob() {
    if (T) (void)hipFree(T);
  }
};

// the group pass and the scans: j.rows / j.segs of the job (nothing is written to the caller)
int read_size(JgReadJob& j) {
  jg_engine* e = j.e;
  HIPCHK(hipSetDevice(e->device));
  {
    const int rc = sync_and_check(e);  // (JG_NODE_ASYNC steps settled; everything issued before is in the columns)
    if (rc) return rc;
  }
  if (!j.n) return JG_OK;
  const uint32_t n = j.n, tiles = (n + JG_BLOCK - 1) / JG_BLOCK;
  Carve& c = j.scratch;
  const size_t o_from = c.sect((size_t)n * 8), o_commit = c.sect((size_t)n * 8), o_off = c.sect((size_t)n * 8),
               o_br = c.sect((size_t)tiles * 8), o_bs = c.sect((size_t)tiles * 8), o_total = c.sect(16),
               o_jobs = c.sect(sizeof j.jobs), o_err = c.sect(4), o_has = c.sect(n), o_fault = c.sect(n);
  char* B = nullptr;
  if (const int rc = c.alloc(B)) return rc;
  JgReadArgs& a = j.a;
  a.n = n;
  a.g0 = j.g0;
  a.from = j.from ? (const uint64_t*)(B + o_from) : nullptr;
  a.commit = (uint64_t*)(B + o_commit);
  a.has_commit = (uint8_t*)(B + o_has);
  a.fault = (uint8_t*)(B + o_fault);
  a.bsum_r = (uint64_t*)(B + o_br);
  a.bsum_s = (uint64_t*)(B + o_bs);
  a.total = (uint64_t*)(B + o_total);
  a.off = (uint64_t*)(B + o_off);
  a.err = (uint32_t*)(B + o_err);
  j.jobs[0] = JgScanJob{a.bsum_r, tiles, 0};
  j.jobs[1] = JgScanJob{a.bsum_s, tiles, 0};
  if (j.from) HIPCHK(hipMemcpyAsync(B + o_from, j.from, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(B + o_jobs, j.jobs, sizeof j.jobs, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemsetAsync(B + o_err, 0, 4, e->stream));
  hipLaunchKernelGGL(k_read_groups, dim3(tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
  hipLaunchKernelGGL(k_scan_block_sums, dim3(2), dim3(JG_BLOCK), 0, e->stream, (const JgScanJob*)(B + o_jobs), a.total);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(j.totals, a.total, 16, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(&j.err, a.err, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (j.err) return fail(JG_EINVAL, "jg_engine_read_chains: 2^32 rows or more in one tile of groups: split the range");
  j.rows = j.totals[0];
  j.segs = j.totals[1];
  return JG_OK;
}

// the segment table and the rows: the caller's arrays at the job's group offset and at row offset `row_base`
int read_write(JgReadJob& j, const jg_chain_read* r, uint64_t row_base) {
  jg_engine* e = j.e;
  if (!j.n) return JG_OK;
  HIPCHK(hipSetDevice(e->device));
  const uint32_t n = j.n, gi = j.at, tiles = (n + JG_BLOCK - 1) / JG_BLOCK;
  JgReadArgs& a = j.a;
  a.row_base = row_base;
  if (j.segs) {
    HIPCHK(hipMalloc((void**)&j.T, (size_t)j.segs * 24));
    a.seg_lo = (uint64_t*)j.T;
    a.seg_nx = a.seg_lo + j.segs;
    a.seg_row = a.seg_nx + j.segs;
  }
  hipLaunchKernelGGL(k_read_segs, dim3(tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(r->off + gi, a.off, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(r->commit + gi, a.commit, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(r->has_commit + gi, a.has_commit, n, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(r->fault + gi, a.fault, n, hipMemcpyDeviceToHost, e->stream));
  const uint64_t rows = j.rows;
  if (!rows) {
    HIPCHK(hipStreamSynchronize(e->stream));
    return JG_OK;
  }
  // pieces of JG_READ_PIECE rows, two columns each: a staging buffer holds the largest piece's ids, then its nexts
  const uint64_t P = (rows + JG_READ_PIECE - 1) / JG_READ_PIECE, nb = std::min<uint64_t>(rows, JG_READ_PIECE);
  uint64_t* out_id = r->blk_id + row_base;
  uint64_t* out_nx = r->blk_next + row_base;
  return staged_pieces(
      e, P, (size_t)nb * 16,
      [&](uint64_t k, char* buf) -> int {
        const uint64_t r0 = k * JG_READ_PIECE, nr = std::min<uint64_t>(JG_READ_PIECE, rows - r0);
        hipLaunchKernelGGL(k_read_rows, dim3((uint32_t)((nr + JG_READ_TILE - 1) / JG_READ_TILE)), dim3(JG_BLOCK), 0, e->stream,
                           (const uint64_t*)a.seg_lo, (const uint64_t*)a.seg_nx, (const uint64_t*)a.seg_row, j.segs, r0, nr, (uint64_t*)buf,
                           (uint64_t*)buf + nb);
        HIPCHK(hipGetLastError());
        return JG_OK;
      },
      [&](uint64_t k, const char* buf) -> int {
        const uint64_t r0 = k * JG_READ_PIECE, nr = std::min<uint64_t>(JG_READ_PIECE, rows - r0);
        HIPCHK(hipMemcpyAsync(out_id + r0, buf, nr * 8, hipMemcpyDeviceToHost, e->staging.cs));
        HIPCHK(hipMemcpyAsync(out_nx + r0, (const uint64_t*)buf + nb, nr * 8, hipMemcpyDeviceToHost, e->staging.cs));
        return JG_OK;
      });
}

}  // namespace

extern "C" {

int jg_engine_read_chains(jg_engine* e, jg_chain_read* r, uint64_t* n_rows) {
  if (!e || !r || !n_rows) return fail(JG_EINVAL, "null argument");
  const uint32_t g0 = r->g0, n = r->n;
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_read_chains: group range out of bounds");
  if (!r->off || (n && (!r->commit || !r->has_commit || !r->fault))) return fail(JG_EINVAL, "null argument");
  if (r->cap && (!r->blk_id || !r->blk_next)) return fail(JG_EINVAL, "null argument");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  // every shard's size first - JG_ECAPACITY must leave every output as it was - then each shard writes its part, its
  // rows after those of the shards before it
  const size_t D = shard_count(e);
  std::vector<JgReadJob> jobs(D);
  for (size_t d = 0; d < D; d++) {
    const ShardPart p = shard_part(e, d, g0, n);
    jobs[d].e = shard_at(e, d), jobs[d].g0 = p.g0, jobs[d].n = p.n, jobs[d].at = p.at;
    jobs[d].from = r->from ? r->from + p.at : nullptr;
  }
  int rc = each_shard(e, [&](size_t d) -> int { return read_size(jobs[d]); });
  if (rc) return rc;
  std::vector<uint64_t> base(D + 1, 0);
  for (size_t d = 0; d < D; d++) base[d + 1] = base[d] + jobs[d].rows;
  *n_rows = base[D];
  if (base[D] > r->cap) return fail(JG_ECAPACITY, "jg_engine_read_chains: the rows do not fit cap (*n_rows is set)");
  rc = each_shard(e, [&](size_t d) -> int { return read_write(jobs[d], r, base[d]); });
  if (rc) return rc;
  r->off[n] = base[D];
  return JG_OK;
}

}  // extern "C"
