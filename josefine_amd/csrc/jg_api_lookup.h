// jg_api_lookup.h - jg_engine_lookup_groups: the state of a list of slots in one call (jg_lookup.h).  A call that reads,
// under the rules of jg_api_manage.h: refused while kept node steps are outstanding, JG_NODE_ASYNC steps settled, the rows
// made in the engine's staging.  A list of at most JG_LOOKUP_PIECE entries is one upload, one launch, one or two copies and
// one synchronisation; a longer one goes through staged_pieces, piece k's copy to the caller under piece k + 1's kernel.  A
// multi-device handle partitions a host list by owner shard and scatters the answers back to the order asked.  Part of
// josefine_gpu.hip's one translation unit.
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

}  // namespace

extern "C" {

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
