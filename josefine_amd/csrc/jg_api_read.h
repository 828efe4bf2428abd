// jg_api_read.h - jg_engine_read_chains: each group's chain tree read back out as the CSR rows of a sled scan, the
// inverse of jg_engine_load_chains (jg_api_load.h).  The host sizes the read with the group passes of jg_read.h, checks
// the caller's capacity, then writes the rows piece by piece through two staging buffers: the kernel of piece k + 1
// runs while piece k travels to the caller.  Part of josefine_gpu.hip's one translation unit.
#pragma once

namespace {

// one single-device engine's part of a read: groups [g0, g0 + n) of it; the device scratch lives until the job ends
struct JgReadJob {
  jg_engine* e = nullptr;
  uint32_t g0 = 0, n = 0;
  const uint64_t* from = nullptr;
  uint64_t rows = 0, segs = 0;
  JgReadArgs a{};
  JgScanJob jobs[2]{};
  uint64_t totals[2]{};
  uint32_t err = 0;
  char* B = nullptr;    // per group and per tile
  char* T = nullptr;    // the segment table
  ~JgReadJob() {
    if (e && e->read_stage.cs) (void)hipStreamSynchronize(e->read_stage.cs);
    if (T) (void)hipFree(T);
    if (B) (void)hipFree(B);
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
  size_t at = 0;
  auto sect = [&](size_t bytes) {
    const size_t s = at;
    at = (at + std::max<size_t>(bytes, 16) + 15) & ~size_t(15);
    return s;
  };
  const size_t o_from = sect((size_t)n * 8), o_commit = sect((size_t)n * 8), o_off = sect((size_t)n * 8),
               o_br = sect((size_t)tiles * 8), o_bs = sect((size_t)tiles * 8), o_total = sect(16),
               o_jobs = sect(sizeof j.jobs), o_err = sect(4), o_has = sect(n), o_fault = sect(n);
  HIPCHK(hipMalloc((void**)&j.B, at));
  char* B = j.B;
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

// the segment table and the rows: the caller's arrays at group offset `gi` and row offset `row_base`
int read_write(JgReadJob& j, const jg_chain_read* r, uint32_t gi, uint64_t row_base) {
  jg_engine* e = j.e;
  if (!j.n) return JG_OK;
  HIPCHK(hipSetDevice(e->device));
  const uint32_t n = j.n, tiles = (n + JG_BLOCK - 1) / JG_BLOCK;
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
  if (rows) {
    // pieces of JG_READ_PIECE rows through two staging buffers: piece k is made on the engine's stream into buffer
    // k & 1 and copied out on a stream of its own; piece k + 2 waits for that copy before it reuses the buffer
    const uint64_t P = (rows + JG_READ_PIECE - 1) / JG_READ_PIECE, nb = std::min<uint64_t>(rows, JG_READ_PIECE);
    jg_engine::ReadStage& st = e->read_stage;
    if (st.bytes < (size_t)nb * 32) {  // two buffers of two columns, grown to the largest piece so far (<= JG_READ_PIECE rows)
      if (st.buf) HIPCHK(hipFree(st.buf));
      st.buf = nullptr, st.bytes = 0;
      HIPCHK(hipMalloc((void**)&st.buf, (size_t)nb * 32));
      st.bytes = (size_t)nb * 32;
    }
    const uint64_t half = st.bytes / 32;  // rows per buffer and column (>= nb)
    uint64_t* st_id[2] = {(uint64_t*)st.buf, (uint64_t*)st.buf + 2 * half};
    uint64_t* st_nx[2] = {(uint64_t*)st.buf + half, (uint64_t*)st.buf + 3 * half};
    if (!st.cs) {
      HIPCHK(hipStreamCreateWithFlags(&st.cs, hipStreamNonBlocking));
      for (uint32_t b = 0; b < 2; b++) {
        HIPCHK(hipEventCreateWithFlags(&st.ev_k[b], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&st.ev_c[b], hipEventDisableTiming));
      }
    }
    uint64_t* out_id = r->blk_id + row_base;
    uint64_t* out_nx = r->blk_next + row_base;
    auto make = [&](uint64_t k) -> int {
      const uint32_t b = (uint32_t)(k & 1);
      const uint64_t r0 = k * JG_READ_PIECE, nr = std::min<uint64_t>(JG_READ_PIECE, rows - r0);
      if (k >= 2) HIPCHK(hipStreamWaitEvent(e->stream, st.ev_c[b], 0));
      hipLaunchKernelGGL(k_read_rows, dim3((uint32_t)((nr + JG_READ_TILE - 1) / JG_READ_TILE)), dim3(JG_BLOCK), 0, e->stream,
                         (const uint64_t*)a.seg_lo, (const uint64_t*)a.seg_nx, (const uint64_t*)a.seg_row, j.segs, r0, nr, st_id[b],
                         st_nx[b]);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(st.ev_k[b], e->stream));
      return JG_OK;
    };
    auto copy = [&](uint64_t k) -> int {
      const uint32_t b = (uint32_t)(k & 1);
      const uint64_t r0 = k * JG_READ_PIECE, nr = std::min<uint64_t>(JG_READ_PIECE, rows - r0);
      HIPCHK(hipStreamWaitEvent(st.cs, st.ev_k[b], 0));
      HIPCHK(hipMemcpyAsync(out_id + r0, st_id[b], nr * 8, hipMemcpyDeviceToHost, st.cs));
      HIPCHK(hipMemcpyAsync(out_nx + r0, st_nx[b], nr * 8, hipMemcpyDeviceToHost, st.cs));
      HIPCHK(hipEventRecord(st.ev_c[b], st.cs));
      return JG_OK;
    };
    int rc = make(0);
    // (a copy into pageable memory may return only when it is done: the next piece's kernel is queued before it)
    for (uint64_t k = 1; k < P && !rc; k++)
      if (!(rc = make(k))) rc = copy(k - 1);
    if (!rc) rc = copy(P - 1);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(st.cs));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return JG_OK;
}

}  // namespace

extern "C" {

int jg_engine_read_chains(jg_engine* e, jg_chain_read* r, uint64_t* n_rows) {
  if (!e || !r || !n_rows) return fail(JG_EINVAL, "null argument");
  const uint32_t g0 = r->g0, n = r->n;
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_read_chains: group range out of bounds");
  if (!r->off || (n && (!r->commit || !r->has_commit || !r->fault))) return fail(JG_EINVAL, "null argument");
  if (r->cap && (!r->blk_id || !r->blk_next)) return fail(JG_EINVAL, "null argument");
  if (!e->router) {
    const int rc0 = kept_refuse(e);
    if (rc0) return rc0;
    JgReadJob j;
    j.e = e, j.g0 = g0, j.n = n, j.from = r->from;
    int rc = read_size(j);
    if (rc) return rc;
    *n_rows = j.rows;
    if (j.rows > r->cap) return fail(JG_ECAPACITY, "jg_engine_read_chains: the rows do not fit cap (*n_rows is set)");
    if ((rc = read_write(j, r, 0, 0))) return rc;
    r->off[n] = j.rows;
    return JG_OK;
  }
  // a sharded handle: every shard's refusal and size first - JG_ECAPACITY must leave every output as it was - then each
  // shard writes its part, its rows after those of the shards before it
  JgRouter& R = *e->router;
  for (jg_engine* s : R.sh) {
    const int rc = kept_refuse(s);
    if (rc) return rc;
  }
  std::vector<JgReadJob> jobs(R.D());
  for (size_t d = 0; d < R.D(); d++) {
    const uint32_t a = std::max<uint32_t>(g0, R.lo[d]), b = std::min<uint32_t>(g0 + n, R.lo[d + 1]);
    jobs[d].e = R.sh[d];
    if (a >= b) continue;
    jobs[d].g0 = a - R.lo[d], jobs[d].n = b - a;
    jobs[d].from = r->from ? r->from + (a - g0) : nullptr;
  }
  int rc = R.run([&](size_t d) { return read_size(jobs[d]); });
  if (rc) return rc;
  std::vector<uint64_t> base(R.D() + 1, 0);
  for (size_t d = 0; d < R.D(); d++) base[d + 1] = base[d] + jobs[d].rows;
  *n_rows = base[R.D()];
  if (base[R.D()] > r->cap) return fail(JG_ECAPACITY, "jg_engine_read_chains: the rows do not fit cap (*n_rows is set)");
  rc = R.run([&](size_t d) {
    const uint32_t a = std::max<uint32_t>(g0, R.lo[d]);
    return read_write(jobs[d], r, jobs[d].n ? a - g0 : 0, base[d]);
  });
  if (rc) return rc;
  r->off[n] = base[R.D()];
  return JG_OK;
}

}  // extern "C"
