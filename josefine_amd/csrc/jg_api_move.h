// jg_api_move.h - jg_engine_export_groups / jg_engine_import_groups: live groups handed between engines through a state
// image (jg_move.h), without a restart.  A host-form export streams pieces of records through the engine's staging
// (jg_api_manage.h's staged_pieces): the kernel of piece k + 1 runs while piece k travels to the caller.  A host-form
// import uploads the whole image into device scratch, validates every record (k_import_check) and only then scatters it
// into the columns (k_import_groups): jg_api_manage.h's check_then_write.  Part of josefine_gpu.hip's one translation unit.
#pragma once

#define JG_MOVE_PIECE (1u << 18)  // records per staging piece of a host-form export (a multiple of JG_MOVE_TILE)

namespace {

uint32_t move_record_bytes(const jg_engine* e) { return jg_move_words(e->cfg.n_replicas) * 8u; }

void move_header(const jg_engine* e, uint32_t g0, uint32_t n, jg_group_image_header* h) {
  *h = jg_group_image_header{};
  h->format = JG_MOVE_FORMAT;
  h->record_bytes = move_record_bytes(e);
  h->n = n;
  h->n_replicas = e->cfg.n_replicas;
  for (uint32_t r = 0; r < e->cfg.n_replicas; r++) h->node_ids[r] = e->cfg.node_ids[r];
  h->separate_commit_key = (e->cfg.flags & JG_CFG_SEPARATE_COMMIT_KEY) ? 1u : 0u;
  h->seed = e->cfg.seed;
  h->global0 = e->cfg.group_base + g0;
}

// the header of an image against the engine it is to be imported into (slots must mean the same nodes)
int move_check_header(const jg_engine* e, const jg_group_image_header& h) {
  if (h.format != JG_MOVE_FORMAT) return fail(JG_EINVAL, "jg_engine_import_groups: unknown image format");
  if (h.n_replicas != e->cfg.n_replicas) return fail(JG_EINVAL, "jg_engine_import_groups: the image's n_replicas differs from the engine's");
  if (h.record_bytes != move_record_bytes(e)) return fail(JG_EINVAL, "jg_engine_import_groups: record_bytes mismatch");
  for (uint32_t r = 0; r < e->cfg.n_replicas; r++)
    if (h.node_ids[r] != e->cfg.node_ids[r]) return fail(JG_EINVAL, "jg_engine_import_groups: the image's node_ids differ from the engine's");
  if ((h.separate_commit_key != 0) != ((e->cfg.flags & JG_CFG_SEPARATE_COMMIT_KEY) != 0))
    return fail(JG_EINVAL, "jg_engine_import_groups: JG_CFG_SEPARATE_COMMIT_KEY differs from the engine's");
  return JG_OK;
}

// one single-device engine's part of an export: groups [g0, g0 + n) into `dst` (host memory, or the device's own)
int export_shard(jg_engine* e, uint32_t g0, uint32_t n, char* dst, bool device) {
  HIPCHK(hipSetDevice(e->device));
  {
    const int rc = sync_and_check(e);  // (JG_NODE_ASYNC steps settled: everything issued before is in the columns)
    if (rc) return rc;
  }
  if (!n) return JG_OK;
  if (device) {
    JgMoveArgs a{};
    a.g0 = g0, a.n = n, a.out = (uint4*)dst;
    JG_LAUNCH_RECORDS(k_export_groups, e, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return JG_OK;
  }
  // pieces of JG_MOVE_PIECE records
  const size_t S = move_record_bytes(e);
  const uint32_t P = (n + JG_MOVE_PIECE - 1) / JG_MOVE_PIECE, np = std::min<uint32_t>(n, JG_MOVE_PIECE);
  return staged_pieces(
      e, P, np * S,
      [&](uint64_t k, char* buf) -> int {
        const uint32_t r0 = (uint32_t)k * JG_MOVE_PIECE;
        JgMoveArgs p{};
        p.g0 = g0 + r0, p.n = std::min<uint32_t>(JG_MOVE_PIECE, n - r0), p.out = (uint4*)buf;
        JG_LAUNCH_RECORDS(k_export_groups, e, p);
        HIPCHK(hipGetLastError());
        return JG_OK;
      },
      [&](uint64_t k, const char* buf) -> int {
        const uint32_t r0 = (uint32_t)k * JG_MOVE_PIECE, nr = std::min<uint32_t>(JG_MOVE_PIECE, n - r0);
        HIPCHK(hipMemcpyAsync(dst + (size_t)r0 * S, buf, (size_t)nr * S, hipMemcpyDeviceToHost, e->staging.cs));
        return JG_OK;
      });
}

// one single-device engine's part of an import: staged and validated first (check), written only when every part has
// passed (write).  The device scratch lives until the job ends.
struct JgImportJob {
  jg_engine* e = nullptr;
  uint32_t g0 = 0, n = 0;
  const char* src = nullptr;  // the part's first record (host, or the device's own memory)
  bool device = false;
  uint64_t shift = 0;
  char* B = nullptr;          // [n] records (host form) + the error words
  uint32_t* d_err = nullptr;
  uint32_t err[2] = {0, 0};
  ~JgImportJob() {
    if (B) (void)hipFree(B);
  }
};

JgMoveArgs import_args(const JgImportJob& j) {
  JgMoveArgs a{};
  a.g0 = j.g0, a.n = j.n, a.shift = j.shift, a.err = j.d_err;
  a.in = (const uint4*)(j.device ? j.src : j.B);
  return a;
}

int import_check(JgImportJob& j) {
  jg_engine* e = j.e;
  if (!j.n) return JG_OK;
  HIPCHK(hipSetDevice(e->device));
  {
    const int rc = node_settle(e);
    if (rc) return rc;
  }
  const size_t S = move_record_bytes(e), img = j.device ? 0 : (size_t)j.n * S;
  HIPCHK(hipMalloc((void**)&j.B, img + 16));
  j.d_err = (uint32_t*)(j.B + img);
  if (!j.device) HIPCHK(hipMemcpyAsync(j.B, j.src, img, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemsetAsync(j.d_err, 0, 8, e->stream));
  const JgMoveArgs a = import_args(j);
  JG_LAUNCH_RECORDS(k_import_check, e, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(j.err, j.d_err, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (j.err[0] & 2u) return fail(JG_EDEVICE, "internal: jg_engine_import_groups met per-step deferral bits of a destination group between calls (nothing was imported)");
  if (j.err[0]) return fail(JG_EINVAL, "jg_engine_import_groups: a record failed its check word or a field is out of range (nothing was imported)");
  return JG_OK;
}

int import_write(JgImportJob& j) {
  jg_engine* e = j.e;
  if (!j.n) return JG_OK;
  HIPCHK(hipSetDevice(e->device));
  const JgMoveArgs a = import_args(j);
  JG_LAUNCH_RECORDS(k_import_groups, e, a);
  HIPCHK(hipGetLastError());
  groups_rewritten(e, j.err[1]);  // (err[1]: the mask of the own slots among the records, from the check pass)
  HIPCHK(hipStreamSynchronize(e->stream));  // (the pageable source and the scratch are done with)
  return JG_OK;
}

}  // namespace

extern "C" {

int jg_engine_export_groups(jg_engine* e, jg_group_export* x) {
  if (!e || !x) return fail(JG_EINVAL, "null argument");
  const uint32_t g0 = x->g0, n = x->n;
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_export_groups: group range out of bounds");
  const bool device = (x->flags & JG_MOVE_DEVICE) != 0;
  if (device && e->router) return fail(JG_EINVAL, "jg_engine_export_groups: device records are per shard: the host form on a multi-device handle");
  if (device && ((uintptr_t)x->records & 15u)) return fail(JG_EINVAL, "jg_engine_export_groups: device records must be 16-byte aligned");
  move_header(e, g0, n, &x->header);
  const size_t S = move_record_bytes(e);
  if ((uint64_t)n * S > x->cap_bytes) return fail(JG_ECAPACITY, "jg_engine_export_groups: the records do not fit cap_bytes (the header is set)");
  if (n && !x->records) return fail(JG_EINVAL, "null argument");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  return each_shard(e, [&](size_t d) -> int {
    const ShardPart p = shard_part(e, d, g0, n);  // (a shard that owns none of the range still settles its steps)
    return export_shard(shard_at(e, d), p.g0, p.n, (char*)x->records + (size_t)p.at * S, device);
  });
}

int jg_engine_import_groups(jg_engine* e, const jg_group_import* x) {
  if (!e || !x) return fail(JG_EINVAL, "null argument");
  const uint32_t g0 = x->g0, n = x->header.n;
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_import_groups: group range out of bounds");
  {
    const int rc = move_check_header(e, x->header);
    if (rc) return rc;
  }
  const bool device = (x->flags & JG_MOVE_DEVICE) != 0;
  if (device && e->router) return fail(JG_EINVAL, "jg_engine_import_groups: device records are per shard: the host form on a multi-device handle");
  if (device && ((uintptr_t)x->records & 15u)) return fail(JG_EINVAL, "jg_engine_import_groups: device records must be 16-byte aligned");
  if (n && !x->records) return fail(JG_EINVAL, "null argument");
  if (const int rc = refuse_first(e, rewrite_refuse)) return rc;
  const size_t S = move_record_bytes(e);
  return check_then_write<JgImportJob>(
      e,
      [&](size_t d, JgImportJob& j) {
        const ShardPart p = shard_part(e, d, g0, n);
        j.e = shard_at(e, d), j.g0 = p.g0, j.n = p.n, j.device = device, j.shift = (uint64_t)x->shift_ms;
        j.src = (const char*)x->records + (size_t)p.at * S;
      },
      import_check, import_write);
}

}  // extern "C"
