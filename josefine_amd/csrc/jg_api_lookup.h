// jg_api_lookup.h - jg_engine_lookup_groups: the state of a list of slots in one call (jg_lookup.h).  A call that reads,
// under the rules of jg_api_manage.h: refused while kept node steps are outstanding, JG_NODE_ASYNC steps settled, the rows
// made in the engine's staging.  A list of at most JG_LOOKUP_PIECE entries is one upload, one launch, one or two copies and
// one synchronisation; a longer one goes through staged_pieces, piece k's copy to the caller under piece k + 1's kernel.  A
// multi-device handle partitions a host list by owner shard and scatters the answers back to the order asked.  Part of
// josefine_gpu.hip's one translation unit.
//
// And jg_step_node_looked / jg_node_lookup_view (ABI v25): the point query that travels with a kept node step, as the poll
// and the completion request do (jg_api_poll.h, jg_api_await.h) - node_lookup_check by the entry point, then
// node_lookup_stage / node_lookup_tail / node_lookup_finish, called by jg_api_node.h.  One piece, one launch of
// k_lookup_kept under the step's general-row gate, the copies home sized exactly: n is known at entry.
#pragma once

#define JG_LOOKUP_PIECE 65536u  // entries per staging piece: two pieces of rows, progress heads and list are 19 MiB at R = 8

namespace {

// where a piece of `np` entries keeps its rows, its progress heads, its part of a host list and the error word
struct LookupPiece {
  size_t rows = 0, match = 0, list = 0, err = 0, bytes = 0;
  LookupPiece(size_t np, uint32_t R, bool progress, bool host_list) {
    Carve c;
    rows = c.sect(np * sizeof(jg_group_state));
    if (progress) match = c.sect(np * R * 8);
    if (host_list) list = c.sect(np * 4);
    err = c.sect(4);
    bytes = c.at;
  }
};

int lookup_launch(jg_engine* e, const JgLookupArgs& a) {
  const dim3 grid((a.n + JG_BLOCK - 1) / JG_BLOCK), block(JG_BLOCK);
  switch (e->cfg.n_replicas) {
    case 1: hipLaunchKernelGGL(k_lookup<1>, grid, block, 0, e->stream, e->dev, a); break;
    case 2: hipLaunchKernelGGL(k_lookup<2>, grid, block, 0, e->stream, e->dev, a); break;
    case 3: hipLaunchKernelGGL(k_lookup<3>, grid, block, 0, e->stream, e->dev, a); break;
    case 4: hipLaunchKernelGGL(k_lookup<4>, grid, block, 0, e->stream, e->dev, a); break;
    case 5: hipLaunchKernelGGL(k_lookup<5>, grid, block, 0, e->stream, e->dev, a); break;
    case 6: hipLaunchKernelGGL(k_lookup<6>, grid, block, 0, e->stream, e->dev, a); break;
    case 7: hipLaunchKernelGGL(k_lookup<7>, grid, block, 0, e->stream, e->dev, a); break;
    default: hipLaunchKernelGGL(k_lookup<8>, grid, block, 0, e->stream, e->dev, a); break;
  }
  HIPCHK(hipGetLastError());
  e->n_launch++;
  return JG_OK;
}

// one single-device engine's part of a lookup: the n entries of `list` (shard-local indices in host memory, or with
// `device` in the engine's own; nullptr: the slots g0 .. g0 + n - 1) as rows (groups + add) into host `out`, their progress
// heads into host `match` (nullptr: none).  A host list has been checked by the caller; a device list is checked here,
// before anything is copied out.
int lookup_shard(jg_engine* e, const uint32_t* list, bool device, uint32_t g0, uint32_t n, uint32_t add, jg_group_state* out, uint64_t* match) {
  if (!n) return JG_OK;
  HIPCHK(hipSetDevice(e->device));
  {
    const int rc = node_settle(e);
    if (rc) return rc;
  }
  const uint32_t R = e->cfg.n_replicas, np = std::min<uint32_t>(n, JG_LOOKUP_PIECE);
  const bool host_list = list && !device;
  const LookupPiece p(np, R, match != nullptr, host_list);
  // piece k's kernel (behind the upload of its part of a host list) into the piece at `buf`
  auto make = [&](uint64_t k, char* buf) -> int {
    const uint64_t r0 = k * JG_LOOKUP_PIECE;
    JgLookupArgs a{};
    a.g0 = g0 + (uint32_t)r0, a.n = (uint32_t)std::min<uint64_t>(JG_LOOKUP_PIECE, n - r0), a.add = add;
    a.list = host_list ? (const uint32_t*)(buf + p.list) : list ? list + r0 : nullptr;
    a.out = (uint4*)(buf + p.rows);
    a.match = match ? (uint64_t*)(buf + p.match) : nullptr;
    a.err = (uint32_t*)(buf + p.err);
    if (host_list) HIPCHK(hipMemcpyAsync(buf + p.list, list + r0, (size_t)a.n * 4, hipMemcpyHostToDevice, e->stream));
    return lookup_launch(e, a);
  };
  // ... and its copies to the caller, queued on `s`
  auto send = [&](uint64_t k, const char* buf, hipStream_t s) -> int {
    const uint64_t r0 = k * JG_LOOKUP_PIECE, nr = std::min<uint64_t>(JG_LOOKUP_PIECE, n - r0);
    HIPCHK(hipMemcpyAsync(out + r0, buf + p.rows, nr * sizeof(jg_group_state), hipMemcpyDeviceToHost, s));
    if (match) HIPCHK(hipMemcpyAsync(match + r0 * R, buf + p.match, nr * R * 8, hipMemcpyDeviceToHost, s));
    return JG_OK;
  };
  const char* refused = "jg_engine_lookup_groups: a slot index of the device list is out of range (nothing was written)";
  if (n <= JG_LOOKUP_PIECE) {
    if (const int rc = e->staging.reserve(p.bytes)) return rc;
    char* B = e->staging.buf;
    uint32_t err = 0;
    if (device) HIPCHK(hipMemsetAsync(B + p.err, 0, 4, e->stream));
    if (const int rc = make(0, B)) return rc;
    if (!device) {
      const int rc = send(0, B, e->stream);
      HIPCHK(hipStreamSynchronize(e->stream));
      return rc;
    }
    // a device list: the error word at the call's one synchronisation, and only then the copies to the caller
    HIPCHK(hipMemcpyAsync(&err, B + p.err, 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (err) return fail(JG_EINVAL, refused);
    HIPCHK(hipMemcpy(out, B + p.rows, (size_t)n * sizeof(jg_group_state), hipMemcpyDeviceToHost));
    if (match) HIPCHK(hipMemcpy(match, B + p.match, (size_t)n * R * 8, hipMemcpyDeviceToHost));
    return JG_OK;
  }
  if (device) {  // every entry's bounds before the first piece leaves for the caller
    if (const int rc = e->staging.reserve(16)) return rc;
    uint32_t* d_err = (uint32_t*)e->staging.buf;
    uint32_t err = 0;
    HIPCHK(hipMemsetAsync(d_err, 0, 4, e->stream));
    hipLaunchKernelGGL(k_lookup_check, dim3(std::min<uint32_t>((n + JG_BLOCK - 1) / JG_BLOCK, 2048u)), dim3(JG_BLOCK), 0, e->stream,
                       e->cfg.n_groups, list, (uint64_t)n, d_err);
    HIPCHK(hipGetLastError());
    e->n_launch++;
    HIPCHK(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (err) return fail(JG_EINVAL, refused);
  }
  const uint64_t P = ((uint64_t)n + JG_LOOKUP_PIECE - 1) / JG_LOOKUP_PIECE;
  return staged_pieces(e, P, p.bytes, make, [&](uint64_t k, const char* buf) -> int { return send(k, buf, e->staging.cs); });
}

// ---- a point query behind a kept node step (jg_step_node_looked) -------------------------------------------------------
static_assert(JG_NODE_LOOKUP_MAX == JG_LOOKUP_PIECE, "a looked step carries one staging piece");

// the rules of jg_step_node_looked for *s on a single-device engine; `lk`: what the step's set keeps of it
int node_lookup_check(const jg_engine* e, const jg_group_set* s, jg_engine::NodeLookup& lk) {
  const uint32_t G = e->cfg.n_groups;
  if (s->flags & ~(uint32_t)(JG_GROUPS_DEVICE | JG_LOOKUP_PROGRESS)) return fail(JG_EINVAL, "jg_step_node_looked: unknown flag");
  if (s->flags & JG_GROUPS_DEVICE) return fail(JG_EINVAL, "jg_step_node_looked: a device list's bounds are known only on the device: a host list or a range");
  if (s->self_slots) return fail(JG_EINVAL, "jg_step_node_looked: self_slots must be null");
  if (s->n > JG_NODE_LOOKUP_MAX) return fail(JG_EINVAL, "jg_step_node_looked: more than JG_NODE_LOOKUP_MAX entries");
  if (!s->groups && (uint64_t)s->g0 + s->n > G) return fail(JG_EINVAL, "jg_step_node_looked: slot range out of bounds");
  if (s->groups)
    for (uint32_t i = 0; i < s->n; i++)
      if (s->groups[i] >= G) return fail(JG_EINVAL, "jg_step_node_looked: a slot index is out of range (nothing was stepped)");
  lk = jg_engine::NodeLookup{};
  lk.on = true, lk.g0 = s->groups ? 0u : s->g0, lk.n = s->n;
  lk.progress = (s->flags & JG_LOOKUP_PROGRESS) != 0, lk.listed = s->groups != nullptr;
  return JG_OK;
}

// where the answer of n entries lands in the set's pinned area: the rows, the progress heads, the header words
LookupPiece node_lookup_landing(const jg_engine* e, const jg_engine::NodeLookup& lk) { return LookupPiece(lk.n, e->cfg.n_replicas, lk.progress, false); }

// the step's list into the set's pinned staging, and the landing area at its size (the set is the step's from here on:
// whatever read it last has been viewed, and the pointers of that view went with the claim)
int node_lookup_stage(jg_engine* e, jg_engine::NodeOut& o, const uint32_t* list) {
  const jg_engine::NodeLookup& lk = o.lk;
  o.l_lookup_up.n = o.l_lookup.n = 0;
  const LookupPiece land = node_lookup_landing(e, lk);
  HIPCHK(o.l_lookup.reserve(land.bytes));
  std::memset(o.l_lookup.p + land.err, 0xff, JG_LH_WORDS * 4);  // (nothing has landed: a header that never arrives is a gated one)
  if (lk.listed && lk.n) {
    HIPCHK(o.l_lookup_up.reserve((size_t)lk.n * 4));
    std::memcpy(o.l_lookup_up.p, list, (size_t)lk.n * 4);
  }
  return JG_OK;
}

int node_lookup_launch(jg_engine* e, const JgLookupArgs& a, const uint32_t* gate, uint32_t* hdr) {
  const dim3 grid((a.n + JG_BLOCK - 1) / JG_BLOCK), block(JG_BLOCK);
  switch (e->cfg.n_replicas) {
    case 1: hipLaunchKernelGGL(k_lookup_kept<1>, grid, block, 0, e->stream, e->dev, a, gate, hdr); break;
    case 2: hipLaunchKernelGGL(k_lookup_kept<2>, grid, block, 0, e->stream, e->dev, a, gate, hdr); break;
    case 3: hipLaunchKernelGGL(k_lookup_kept<3>, grid, block, 0, e->stream, e->dev, a, gate, hdr); break;
    case 4: hipLaunchKernelGGL(k_lookup_kept<4>, grid, block, 0, e->stream, e->dev, a, gate, hdr); break;
    case 5: hipLaunchKernelGGL(k_lookup_kept<5>, grid, block, 0, e->stream, e->dev, a, gate, hdr); break;
    case 6: hipLaunchKernelGGL(k_lookup_kept<6>, grid, block, 0, e->stream, e->dev, a, gate, hdr); break;
    case 7: hipLaunchKernelGGL(k_lookup_kept<7>, grid, block, 0, e->stream, e->dev, a, gate, hdr); break;
    default: hipLaunchKernelGGL(k_lookup_kept<8>, grid, block, 0, e->stream, e->dev, a, gate, hdr); break;
  }
  HIPCHK(hipGetLastError());
  e->n_launch++;
  return JG_OK;
}

// The point query of kept step `o`, queued behind the kernels of that step (its poll and its completion request) that are
// in the stream by now, and its trip home on the down stream: the rows, the progress heads and the header words, each one
// copy of exactly its size.  Scratch - list, rows, heads, header - is the set's arena's: the engine's staging may be carved
// again by a later call while this answer is still on its way.  The first pass sends the staged list up, behind the step.
// `gate`: as for node_poll_tail.  Synchronises nothing.
int node_lookup_tail(jg_engine* e, jg_engine::NodeOut& o, const uint32_t* gate) {
  jg_engine::NodeStep& nd = e->node;
  jg_engine::NodeLookup& lk = o.lk;
  if (!lk.n) return JG_OK;
  const uint32_t R = e->cfg.n_replicas;
  const LookupPiece p(lk.n, R, lk.progress, lk.listed), land = node_lookup_landing(e, lk);
  if (!lk.scratch) HIPCHK(e->arenas[o.arena].alloc(p.bytes, (void**)&lk.scratch));  // (the pass behind the catch-up pass: the same block)
  char* const B = lk.scratch;
  uint32_t* const hdr = (uint32_t*)(B + p.err);
  if (!lk.redone) {
    if (lk.listed) HIPCHK(hipMemcpyAsync(B + p.list, o.l_lookup_up.p, (size_t)lk.n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(hdr, 0, 16, e->stream));  // (the error word is only ever raised)
  }
  JgLookupArgs a{};
  a.g0 = lk.g0, a.n = lk.n, a.add = 0;
  a.list = lk.listed ? (const uint32_t*)(B + p.list) : nullptr;
  a.out = (uint4*)(B + p.rows);
  a.match = lk.progress ? (uint64_t*)(B + p.match) : nullptr;
  a.err = hdr + JG_LH_ERR;
  if (const int rc = node_lookup_launch(e, a, gate, hdr)) return rc;
  HIPCHK(hipEventRecord(o.ev_kernels, e->stream));
  HIPCHK(hipStreamWaitEvent(nd.down, o.ev_kernels, 0));
  char* const L = o.l_lookup.p;
  HIPCHK(hipMemcpyAsync(L + land.rows, B + p.rows, (size_t)lk.n * sizeof(jg_group_state), hipMemcpyDeviceToHost, nd.down));
  if (lk.progress) HIPCHK(hipMemcpyAsync(L + land.match, B + p.match, (size_t)lk.n * R * 8, hipMemcpyDeviceToHost, nd.down));
  HIPCHK(hipMemcpyAsync(L + land.err, hdr, JG_LH_WORDS * 4, hipMemcpyDeviceToHost, nd.down));
  return JG_OK;
}

// Kept step `o` is being viewed and its outputs have landed: the header words say whether the rows are an answer - a pass
// that was gated and never queued again left none - and the landing pointers are what jg_node_lookup_view hands out from
// here on.  Before the set's arena starts over.
int node_lookup_finish(jg_engine* e, jg_engine::NodeOut& o) {
  jg_engine::NodeLookup& lk = o.lk;
  jg_node_lookup& v = o.lookup_view;
  v = jg_node_lookup{};
  if (!lk.on) return JG_OK;
  lk.scratch = nullptr;  // (the arena's: gone with it)
  const LookupPiece land = node_lookup_landing(e, lk);
  const uint32_t* const h = (const uint32_t*)(o.l_lookup.p + land.err);
  if (lk.n && h[JG_LH_GATE]) return fail(JG_EDEVICE, "internal: a looked step's pass was gated and not queued again");
  if (lk.n && h[JG_LH_ERR]) return fail(JG_EDEVICE, "internal: a looked step's list held an index out of range");
  v.rows = (const jg_group_state*)(o.l_lookup.p + land.rows);  // (no entries: the pointers are the area's all the same)
  v.match = lk.progress ? (const uint64_t*)(o.l_lookup.p + land.match) : nullptr;
  v.attached = 1u, v.state = lk.redone ? (uint32_t)JG_NODE_POLL_REDONE : 0u;
  v.n = lk.n;
  return JG_OK;
}

}  // namespace

extern "C" {

int jg_node_lookup_view(jg_engine* e, jg_node_lookup* out) {
  if (!e || !out) return fail(JG_EINVAL, "null argument");
  if (e->router) return fail(JG_EINVAL, "jg_node_lookup_view: a looked step is a shard's (jg_get_shard)");
  if (e->node.poll_viewed < 0) return fail(JG_EINVAL, "jg_node_lookup_view: no kept step's outbox has been viewed (or a newer step has claimed its set)");
  *out = e->node.sets[e->node.poll_viewed].lookup_view;
  return JG_OK;
}

int jg_engine_lookup_groups(jg_engine* e, const jg_group_set* s, jg_group_state* out, uint64_t* match) {
  if (!e || !s) return fail(JG_EINVAL, "null argument");
  const uint32_t n = s->n, G = e->cfg.n_groups, R = e->cfg.n_replicas;
  if (n && !out) return fail(JG_EINVAL, "null argument");
  if (s->flags & ~(uint32_t)(JG_GROUPS_DEVICE | JG_LOOKUP_PROGRESS)) return fail(JG_EINVAL, "jg_engine_lookup_groups: unknown flag");
  const bool device = (s->flags & JG_GROUPS_DEVICE) != 0, progress = (s->flags & JG_LOOKUP_PROGRESS) != 0;
  if (progress && !match) return fail(JG_EINVAL, "jg_engine_lookup_groups: JG_LOOKUP_PROGRESS needs `match`");
  const uint32_t* L = s->groups;
  if (!L && (uint64_t)s->g0 + n > G) return fail(JG_EINVAL, "jg_engine_lookup_groups: slot range out of bounds");
  if (device && e->router) return fail(JG_EINVAL, "jg_engine_lookup_groups: device lists are per shard: a host list on a multi-device handle");
  if (L && !device)  // a host list: checked here, before anything is queued
    for (uint32_t i = 0; i < n; i++)
      if (L[i] >= G) return fail(JG_EINVAL, "jg_engine_lookup_groups: a slot index is out of range (nothing was written)");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  if (!n) return JG_OK;
  uint64_t* m = progress ? match : nullptr;
  if (!e->router) return lookup_shard(e, L, device && L, s->g0, n, 0, out, m);  // (straight into the caller's arrays)
  const std::vector<uint32_t>& lo = e->router->lo;
  if (!L)  // a range: every shard's part is a range of the caller's arrays
    return each_shard(e, [&](size_t d) -> int {
      const ShardPart p = shard_part(e, d, s->g0, n);
      return lookup_shard(shard_at(e, d), nullptr, false, p.g0, p.n, lo[d], out + p.at, m ? m + (size_t)p.at * R : nullptr);
    });
  // a list: the entries partitioned by owner shard (stably: a shard answers its entries in the order asked), every shard
  // looks its part up, and the rows and progress heads are scattered back to the caller's order
  const size_t D = shard_count(e);
  std::vector<std::vector<uint32_t>> local(D), at(D);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t d = e->router->owner(L[i]);
    local[d].push_back(L[i] - lo[d]);
    at[d].push_back(i);
  }
  std::vector<std::vector<jg_group_state>> rows(D);
  std::vector<std::vector<uint64_t>> heads(D);
  const int rc = each_shard(e, [&](size_t d) -> int {
    const size_t k = local[d].size();
    rows[d].resize(k);
    if (m) heads[d].resize(k * R);
    return lookup_shard(shard_at(e, d), local[d].data(), false, 0, (uint32_t)k, lo[d], rows[d].data(), m ? heads[d].data() : nullptr);
  });
  if (rc) return rc;
  for (size_t d = 0; d < D; d++)
    for (size_t k = 0; k < at[d].size(); k++) {
      out[at[d][k]] = rows[d][k];
      if (m) std::memcpy(m + (size_t)at[d][k] * R, heads[d].data() + k * R, (size_t)R * 8);
    }
  return JG_OK;
}

}  // extern "C"
