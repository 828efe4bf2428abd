// jg_api_manage.h - what the control-plane families share on the host (jg_api_load.h, jg_api_read.h, jg_api_move.h,
// jg_api_hosting.h): the engine's staging, the piece pipeline of a staged download, the scratch carver, a shard's part of a
// group range, the refusal gate, the check-then-write runner, what a rewrite of group state owes the engine, and the
// dispatch of the record kernels.  A single-device engine is the one-shard case of everything here.  These calls are
// synchronous, so each has the engine's staging to itself from entry to return.  Part of josefine_gpu.hip's one
// translation unit.
#pragma once

// ---- the staging (jg_engine::Staging, jg_api_core.h) ------------------------------------------------------------------

// the buffer holds at least `bytes` (grown, never shrunk: only an engine's first call of a size pays for the allocation)
inline int jg_engine::Staging::reserve(size_t want) {
  if (bytes >= want) return JG_OK;
  if (buf) HIPCHK(hipFree(buf));
  buf = nullptr, bytes = 0;
  HIPCHK(hipMalloc((void**)&buf, want));
  bytes = want;
  return JG_OK;
}

// the copy stream and the four events exist (created at the first staged download)
inline int jg_engine::Staging::streams() {
  if (cs) return JG_OK;
  HIPCHK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  for (hipEvent_t* ev : {&ev_k[0], &ev_k[1], &ev_c[0], &ev_c[1]}) HIPCHK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  return JG_OK;
}

namespace {

// A download of P pieces through the staging, as two buffers of `piece_bytes` (what bounds JG_READ_PIECE and
// JG_MOVE_PIECE: the staging is two buffers of one piece).  launch(k, buf) queues piece k's kernel into its buffer on the
// engine's stream (and checks its launch); copy(k, buf) queues the piece's copies to the caller on the copy stream.
// Piece k uses buffer k & 1; piece k + 2 waits for the copy of piece k before it reuses the buffer.  On every return,
// a failing one included, both streams are idle: nothing travels into the caller's arrays or reads the staging any more.
template <class Launch, class Copy>
int staged_pieces(jg_engine* e, uint64_t P, size_t piece_bytes, Launch launch, Copy copy) {
  jg_engine::Staging& st = e->staging;
  int rc = st.reserve(2 * piece_bytes);
  if (rc || (rc = st.streams())) return rc;
  // `work` queued on `s` behind the event `after` (if any), the event `done` recorded behind it
  auto queue = [&](hipStream_t s, hipEvent_t after, hipEvent_t done, auto work) -> int {
    if (after) HIPCHK(hipStreamWaitEvent(s, after, 0));
    const int rw = work();
    if (rw) return rw;
    HIPCHK(hipEventRecord(done, s));
    return JG_OK;
  };
  auto make = [&](uint64_t k) {
    char* buf = st.buf + (k & 1) * piece_bytes;
    return queue(e->stream, k >= 2 ? st.ev_c[k & 1] : nullptr, st.ev_k[k & 1], [&] { return launch(k, buf); });
  };
  auto send = [&](uint64_t k) {
    const char* buf = st.buf + (k & 1) * piece_bytes;
    return queue(st.cs, st.ev_k[k & 1], st.ev_c[k & 1], [&] { return copy(k, buf); });
  };
  rc = make(0);
  // (a copy into pageable memory may return only when it is done: the next piece's kernel is queued before it)
  for (uint64_t k = 1; k < P && !rc; k++)
    if (!(rc = make(k))) rc = send(k - 1);
  if (!rc) rc = send(P - 1);
  if (rc) {
    (void)hipStreamSynchronize(st.cs), (void)hipStreamSynchronize(e->stream);
    return rc;
  }
  HIPCHK(hipStreamSynchronize(st.cs));
  HIPCHK(hipStreamSynchronize(e->stream));
  return JG_OK;
}

// One scratch block in 16-byte aligned sections: the offsets are handed out first, then the block is allocated once - as
// device memory of its own, freed with the carver, or on the engine's staging.
struct Carve {
  size_t at = 0;
  char* own = nullptr;
  Carve() = default;
  Carve(const Carve&) = delete;
  Carve& operator=(const Carve&) = delete;
  ~Carve() {
    if (own) (void)hipFree(own);
  }
  size_t sect(size_t bytes) {
    const size_t s = at;
    at += (std::max<size_t>(bytes, 16) + 15) & ~size_t(15);
    return s;
  }
  int alloc(char*& B) {
    HIPCHK(hipMalloc((void**)&own, at));
    B = own;
    return JG_OK;
  }
  int on_staging(jg_engine* e, char*& B) {
    const int rc = e->staging.reserve(at);
    B = e->staging.buf;
    return rc;
  }
};

// ---- the engines behind a handle ---------------------------------------------------------------------------------------

inline size_t shard_count(const jg_engine* e) { return e->router ? e->router->D() : 1; }
inline jg_engine* shard_at(jg_engine* e, size_t d) { return e->router ? e->router->sh[d] : e; }

// fn(d) for every shard: each on its device's thread on a multi-device handle (a failure names its shard), else here
template <class F>
int each_shard(jg_engine* e, F fn) {
  return e->router ? e->router->run(fn) : fn(0);
}

// shard d's part of the handle's groups [g0, g0 + n): its shard-local first group, how many (0: none of them), and where
// the part starts in the caller's per-group arrays
struct ShardPart {
  uint32_t g0 = 0, n = 0, at = 0;
};
inline ShardPart shard_part(const jg_engine* e, size_t d, uint32_t g0, uint32_t n) {
  if (!e->router) return {g0, n, 0};
  const std::vector<uint32_t>& lo = e->router->lo;
  const uint32_t a = std::max<uint32_t>(g0, lo[d]), b = std::min<uint32_t>(g0 + n, lo[d + 1]);
  if (a >= b) return {};
  return {a - lo[d], b - a, a - g0};
}

// one shard's W gauge words merged into the handle's: summed, or the larger of the two where is_max(x) says so
template <class IsMax>
void merge_words(uint64_t* dst, const uint64_t* src, uint32_t W, IsMax is_max) {
  for (uint32_t x = 0; x < W; x++) dst[x] = is_max(x) ? std::max(dst[x], src[x]) : dst[x] + src[x];
}
inline bool summed(uint32_t) { return false; }  // (an is_max for words that are all sums)

// ---- refuse first, check, then write -----------------------------------------------------------------------------------

// what refuses a call that rewrites group state before anything is touched (kept_refuse is what refuses one that reads it)
int rewrite_refuse(const jg_engine* e) {
  if (!e->p_kind.empty()) return fail(JG_EINVAL, "commands are queued: call jg_step first");
  return kept_refuse(e);
}

// a refusal applies to every shard before any shard touches anything
int refuse_first(jg_engine* e, int (*refuse)(const jg_engine*)) {
  for (size_t d = 0; d < shard_count(e); d++) {
    const int rc = refuse(shard_at(e, d));
    if (rc) return rc;
  }
  return JG_OK;
}

// write(d) on every shard as ONE step of the handle: the shards' sequence numbers aligned before, the step closed after
template <class Write>
int write_shards(jg_engine* e, Write write) {
  if (e->router) router_align_seq(e);
  const int rc = each_shard(e, write);
  if (e->router) router_after_step(e);
  return rc;
}

// one Job per shard, filled by make(d, job); check(job) on every shard, and only when every one has passed write(job) on
// every shard - one shard cannot refuse after another has written.  A job's device scratch lives until the call ends.
template <class Job, class Make, class Check, class Write>
int check_then_write(jg_engine* e, Make make, Check check, Write write) {
  std::vector<Job> jobs(shard_count(e));
  for (size_t d = 0; d < jobs.size(); d++) make(d, jobs[d]);
  const int rc = each_shard(e, [&](size_t d) -> int { return check(jobs[d]); });
  if (rc) return rc;
  return write_shards(e, [&](size_t d) -> int { return write(jobs[d]); });
}

// What a call that has rewritten group state outside a step owes the engine's summaries of it, as a step keeps them: the
// flag words changed under the dense path's feet, so the device's irregular_seen word is re-read at the next
// synchronisation; and every group has the one own slot `uniform_self`, or the engine stops assuming one
// (own_slots: the mask of the own slots written; 0 when none were).
void groups_rewritten(jg_engine* e, uint32_t own_slots) {
  e->stepped = true;
  e->maybe_irregular = true;
  e->flag_check_pending = true;
  e->irr_gen++;
  if (e->uniform_self >= 0 && (own_slots & ~(1u << e->uniform_self))) e->uniform_self = -1;
}

}  // namespace

// a record kernel of jg_move.h (a tile of JG_MOVE_TILE groups per workgroup) for the engine's record size: 48 or 56 words
#define JG_LAUNCH_RECORDS(kernel, e, a)                                                                            \
  do {                                                                                                             \
    const dim3 grid_(((a).n + JG_MOVE_TILE - 1) / JG_MOVE_TILE);                                                   \
    if (jg_move_words((e)->cfg.n_replicas) == 48)                                                                  \
      hipLaunchKernelGGL(kernel<48>, grid_, dim3(JG_BLOCK), 0, (e)->stream, (e)->dev, a);                          \
    else                                                                                                           \
      hipLaunchKernelGGL(kernel<56>, grid_, dim3(JG_BLOCK), 0, (e)->stream, (e)->dev, a);                          \
    (e)->n_launch++;                                                                                               \
  } while (0)
