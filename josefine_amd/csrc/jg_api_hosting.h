// jg_api_hosting.h - jg_engine_open_groups / jg_engine_close_groups / jg_engine_list_groups: vacant slots (jg_hosting.h).
// Open and close go through jg_api_manage.h's check_then_write: a check pass writes an error word, the host reads it, and
// only then does the write pass run.  The scratch (a host list and its own slots, the error words; the list passes'
// workgroup counts and output) is carved from the engine's staging.  Part of josefine_gpu.hip's one translation unit.
//
// And jg_step_node_hosted / jg_node_hosting_view (ABI v26): the hosting request that travels with a kept node step, as the
// poll, the completion request and the point query do - node_hosting_check by the entry point (jg_api_poll.h), then
// node_hosting_stage / node_hosting_tail / node_hosting_finish, called by jg_api_node.h.  No host read sits between a check
// pass and its write pass there: the kept kernels run under the step's general-row gate, the write pass looks at the error
// word itself, and four header words per set travel home with the step.
#pragma once

namespace {

// one single-device engine's part of an open or a close
struct JgGroupsJob {
  jg_engine* e = nullptr;
  bool open = false, device = false;
  uint32_t g0 = 0, n = 0;
  const uint32_t* list = nullptr;  // shard-local indices (host, or the device's own memory), or nullptr: a range
  const uint8_t* self = nullptr;
  std::vector<uint32_t> local;     // a sharded handle's part of a host list, rebased
  uint64_t now = 0;
  JgGroupsArgs a{};
  uint32_t err[2] = {0, 0};
};

const char* groups_what(const JgGroupsJob& j) { return j.open ? "jg_engine_open_groups" : "jg_engine_close_groups"; }

int groups_check(JgGroupsJob& j) {
  jg_engine* e = j.e;
  if (!j.n) return JG_OK;
  HIPCHK(hipSetDevice(e->device));
  {
    const int rc = node_settle(e);
    if (rc) return rc;
  }
  const bool host_list = j.list && !j.device, host_self = j.self && !j.device;
  Carve c;
  const size_t o_err = c.sect(8), o_list = host_list ? c.sect((size_t)j.n * 4) : 0, o_self = host_self ? c.sect(j.n) : 0;
  char* B = nullptr;
  if (const int rc = c.on_staging(e, B)) return rc;
  j.a = JgGroupsArgs{};
  j.a.g0 = j.g0, j.a.n = j.n, j.a.open = j.open ? 1u : 0u, j.a.seq = e->seq, j.a.now = j.now;
  j.a.err = (uint32_t*)(B + o_err);
  j.a.list = host_list ? (const uint32_t*)(B + o_list) : j.list;
  j.a.self = host_self ? (const uint8_t*)(B + o_self) : j.self;
  if (host_list) HIPCHK(hipMemcpyAsync(B + o_list, j.list, (size_t)j.n * 4, hipMemcpyHostToDevice, e->stream));
  if (host_self) HIPCHK(hipMemcpyAsync(B + o_self, j.self, j.n, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemsetAsync(j.a.err, 0, 8, e->stream));
  hipLaunchKernelGGL(k_groups_check, dim3((j.n + JG_BLOCK - 1) / JG_BLOCK), dim3(JG_BLOCK), 0, e->stream, e->dev, j.a);
  HIPCHK(hipGetLastError());
  e->n_launch++;
  HIPCHK(hipMemcpyAsync(j.err, j.a.err, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  const uint32_t x = j.err[0];
  const std::string w = groups_what(j);
  if (x & JG_HOST_E_RANGE) return fail(JG_EINVAL, w + ": a slot index is out of range (nothing was written)");
  if (x & JG_HOST_E_ORDER) return fail(JG_EINVAL, w + ": the list is not strictly ascending (nothing was written)");
  if (x & JG_HOST_E_SLOT) return fail(JG_EINVAL, w + ": an own slot >= n_replicas (nothing was written)");
  if (x & JG_HOST_E_STATE)
    return fail(JG_EINVAL, w + (j.open ? ": a listed slot already hosts a partition (nothing was written)"
                                       : ": a listed slot is vacant already (nothing was written)"));
  if (x & JG_HOST_E_DEFER) return fail(JG_EDEVICE, "internal: " + w + " met per-step deferral bits of a listed slot between calls (nothing was written)");
  return JG_OK;
}

int groups_write(JgGroupsJob& j) {
  jg_engine* e = j.e;
  if (!j.n) return JG_OK;
  HIPCHK(hipSetDevice(e->device));
  j.a.seq = e->seq;
  const dim3 grid((j.n + JG_BLOCK - 1) / JG_BLOCK);
  if (j.open) hipLaunchKernelGGL(k_groups_open, grid, dim3(JG_BLOCK), 0, e->stream, e->dev, j.a);
  else hipLaunchKernelGGL(k_groups_close, grid, dim3(JG_BLOCK), 0, e->stream, e->dev, j.a);
  HIPCHK(hipGetLastError());
  e->n_launch++;
  groups_rewritten(e, j.open ? j.err[1] : 0);  // (err[1]: the mask of the own slots opened, from the check pass)
  HIPCHK(hipStreamSynchronize(e->stream));  // (the pageable list is done with)
  return JG_OK;
}

int groups_call(jg_engine* e, bool open, uint64_t now_ms, const jg_group_set* s) {
  const char* what = open ? "jg_engine_open_groups" : "jg_engine_close_groups";
  if (!e || !s) return fail(JG_EINVAL, "null argument");
  const bool device = (s->flags & JG_GROUPS_DEVICE) != 0;
  const uint32_t n = s->n, G = e->cfg.n_groups;
  if (!s->groups && (uint64_t)s->g0 + n > G) return fail(JG_EINVAL, std::string(what) + ": slot range out of bounds");
  if (!open && s->self_slots) return fail(JG_EINVAL, "jg_engine_close_groups: self_slots is for opening");
  if (device && e->router) return fail(JG_EINVAL, std::string(what) + ": device lists are per shard: a host list on a multi-device handle");
  if (const int rc = refuse_first(e, rewrite_refuse)) return rc;
  // a sharded handle splits a host list by ownership with one binary search per shard, which needs it ascending and in
  // range: checked here first (the devices check their parts again)
  const uint32_t* L = s->groups;
  const bool split = L && e->router;
  if (split) {
    for (uint32_t i = 0; i < n; i++) {
      if (L[i] >= G) return fail(JG_EINVAL, std::string(what) + ": a slot index is out of range (nothing was written)");
      if (i && L[i - 1] >= L[i]) return fail(JG_EINVAL, std::string(what) + ": the list is not strictly ascending (nothing was written)");
    }
  }
  return check_then_write<JgGroupsJob>(
      e,
      [&](size_t d, JgGroupsJob& j) {
        j.e = shard_at(e, d), j.open = open, j.device = device, j.now = now_ms;
        uint32_t at = 0;  // the part's place in the caller's list and self_slots
        if (split) {
          const std::vector<uint32_t>& lo = e->router->lo;
          at = (uint32_t)(std::lower_bound(L, L + n, lo[d]) - L);
          const uint32_t b = (uint32_t)(std::lower_bound(L, L + n, lo[d + 1]) - L);
          j.local.resize(b - at);
          for (uint32_t i = at; i < b; i++) j.local[i - at] = L[i] - lo[d];
          j.list = j.local.data(), j.n = b - at;
        } else if (L) {
          j.list = L, j.n = n;
        } else {
          const ShardPart p = shard_part(e, d, s->g0, n);
          j.g0 = p.g0, j.n = p.n, at = p.at;
        }
        j.self = s->self_slots ? s->self_slots + at : nullptr;
      },
      groups_check, groups_write);
}

// one single-device engine's part of a list: shard-local slots [g0, g0 + n), the first `cap` matches (indices + add)
// into host `out`; *total the matches
int list_shard(jg_engine* e, uint32_t which, uint32_t g0, uint32_t n, uint32_t add, uint32_t* out, size_t cap, size_t* total) {
  *total = 0;
  if (!n) return JG_OK;
  HIPCHK(hipSetDevice(e->device));
  {
    const int rc = node_settle(e);
    if (rc) return rc;
  }
  const uint32_t tiles = (n + JG_LIST_TILE - 1) / JG_LIST_TILE;
  const size_t wcap = std::min<size_t>(cap, n);
  Carve c;
  const size_t o_total = c.sect(8), o_job = c.sect(sizeof(JgScanJob)), o_bsum = c.sect((size_t)tiles * 8), o_out = c.sect(wcap * 4);
  char* B = nullptr;
  if (const int rc = c.on_staging(e, B)) return rc;
  JgListArgs a{};
  a.g0 = g0, a.n = n, a.which = which, a.add = add;
  a.bsum = (uint64_t*)(B + o_bsum);
  a.out = (uint32_t*)(B + o_out);
  a.cap = wcap;
  const JgScanJob job{a.bsum, tiles, 0};
  HIPCHK(hipMemcpyAsync(B + o_job, &job, sizeof job, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_list_count, dim3(tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
  hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(JG_BLOCK), 0, e->stream, (const JgScanJob*)(B + o_job), (uint64_t*)(B + o_total));
  e->n_launch += 2;
  if (wcap) {
    hipLaunchKernelGGL(k_list_write, dim3(tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
    e->n_launch++;
  }
  HIPCHK(hipGetLastError());
  uint64_t tot = 0;
  HIPCHK(hipMemcpyAsync(&tot, B + o_total, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *total = (size_t)tot;
  const size_t k = std::min<size_t>(wcap, tot);
  if (k) HIPCHK(hipMemcpy(out, a.out, k * 4, hipMemcpyDeviceToHost));
  return JG_OK;
}

// ---- hosting behind a kept node step (jg_step_node_hosted) --------------------------------------------------------------

// the rules of jg_step_node_hosted for one set of the request on a single-device engine; `hs`: what the step's set keeps
int node_hosting_check_set(const jg_engine* e, const jg_group_set* s, bool open, jg_engine::NodeHostSet& hs, uint32_t& own_mask) {
  const uint32_t G = e->cfg.n_groups, R = e->cfg.n_replicas;
  const std::string w = open ? "jg_step_node_hosted: open: " : "jg_step_node_hosted: close: ";
  hs = jg_engine::NodeHostSet{};
  if (!s) return JG_OK;
  if (s->flags & ~(uint32_t)JG_GROUPS_DEVICE) return fail(JG_EINVAL, w + "unknown flag");
  if (s->flags & JG_GROUPS_DEVICE) return fail(JG_EINVAL, w + "a device list's bounds are known only on the device: a host list or a range");
  if (!open && s->self_slots) return fail(JG_EINVAL, w + "self_slots is for opening");
  if ((s->groups || s->self_slots) && s->n > JG_NODE_HOSTING_MAX) return fail(JG_EINVAL, w + "more than JG_NODE_HOSTING_MAX listed entries");
  if (!s->groups && (uint64_t)s->g0 + s->n > G) return fail(JG_EINVAL, w + "slot range out of bounds");
  if (s->groups)
    for (uint32_t i = 0; i < s->n; i++) {
      if (s->groups[i] >= G) return fail(JG_EINVAL, w + "a slot index is out of range (nothing was stepped)");
      if (i && s->groups[i - 1] >= s->groups[i]) return fail(JG_EINVAL, w + "the list is not strictly ascending (nothing was stepped)");
    }
  if (s->self_slots)
    for (uint32_t i = 0; i < s->n; i++) {
      if (s->self_slots[i] >= R) return fail(JG_EINVAL, w + "an own slot >= n_replicas (nothing was stepped)");
      own_mask |= 1u << s->self_slots[i];
    }
  hs.g0 = s->groups ? 0u : s->g0, hs.n = s->n;
  hs.listed = s->groups != nullptr && s->n, hs.own = s->self_slots != nullptr && s->n;
  return JG_OK;
}

int node_hosting_check(const jg_engine* e, const jg_node_hosting_request* req, jg_engine::NodeHosting& hs) {
  hs = jg_engine::NodeHosting{};
  if (const int rc = node_hosting_check_set(e, req->close, false, hs.close, hs.own_mask)) return rc;
  if (const int rc = node_hosting_check_set(e, req->open, true, hs.open, hs.own_mask)) return rc;
  hs.on = true;
  return JG_OK;
}

// where the sets' header words land in the set's pinned area: the close's, then the open's
#define NODE_HOSTING_LAND (2u * JG_HH_WORDS * 4u)

// the step's lists and own slots into the set's pinned staging (the set is the step's from here on: whatever read it last
// has been viewed); the landing area preset to ones - a header that never arrives is a gated one
int node_hosting_stage(jg_engine* e, jg_engine::NodeOut& o, const jg_node_hosting_request* req) {
  (void)e;
  jg_engine::NodeHosting& hs = o.hs;
  Carve c;
  if (hs.close.listed) hs.close.up_list = c.sect((size_t)hs.close.n * 4);
  if (hs.open.listed) hs.open.up_list = c.sect((size_t)hs.open.n * 4);
  if (hs.open.own) hs.open.up_self = c.sect(hs.open.n);
  hs.staged = c.at;
  o.l_hosting_up.n = o.l_hosting.n = 0;
  HIPCHK(o.l_hosting.reserve(NODE_HOSTING_LAND));
  std::memset(o.l_hosting.p, 0xff, NODE_HOSTING_LAND);
  if (c.at) HIPCHK(o.l_hosting_up.reserve(c.at));
  char* const U = o.l_hosting_up.p;
  if (hs.close.listed) std::memcpy(U + hs.close.up_list, req->close->groups, (size_t)hs.close.n * 4);
  if (hs.open.listed) std::memcpy(U + hs.open.up_list, req->open->groups, (size_t)hs.open.n * 4);
  if (hs.open.own) std::memcpy(U + hs.open.up_self, req->open->self_slots, hs.open.n);
  return JG_OK;
}

// The hosting request of kept step `o`, queued behind every kernel of that step that is in the stream by now - its poll's,
// its completion request's, its lookup's - and the header words' trip home on the down stream: check + close, then check +
// open, so that the open's check sees the close's writes; each write pass returns where its check raised the error word.
// Scratch - header words, lists, own slots - is the set's arena's.  The pass behind the catch-up pass uses the same block and
// the step's own step number.  `gate`: as for node_poll_tail.  Synchronises nothing.
int node_hosting_tail(jg_engine* e, jg_engine::NodeOut& o, const uint32_t* gate) {
  jg_engine::NodeStep& nd = e->node;
  jg_engine::NodeHosting& hs = o.hs;
  if (!hs.close.n && !hs.open.n) return JG_OK;
  const size_t staged = hs.staged;
  if (!hs.scratch) {  // (the block: the header words first, then the staging as it was carved)
    HIPCHK(e->arenas[o.arena].alloc(NODE_HOSTING_LAND + staged, (void**)&hs.scratch));
    hs.seq = e->seq;
  }
  char* const B = hs.scratch;
  char* const L = B + NODE_HOSTING_LAND;
  uint32_t* const hdr = (uint32_t*)B;
  if (!hs.redone && staged) HIPCHK(hipMemcpyAsync(L, o.l_hosting_up.p, staged, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemsetAsync(hdr, 0, NODE_HOSTING_LAND, e->stream));  // (the error words are only ever raised, the written words only set)
  for (int open = 0; open < 2; open++) {
    const jg_engine::NodeHostSet& s = open ? hs.open : hs.close;
    if (!s.n) continue;
    uint32_t* const h = hdr + (open ? JG_HH_WORDS : 0u);
    JgGroupsArgs a{};
    a.g0 = s.g0, a.n = s.n, a.open = (uint32_t)open, a.seq = hs.seq, a.now = hs.now;
    a.list = s.listed ? (const uint32_t*)(L + s.up_list) : nullptr;
    a.self = s.own ? (const uint8_t*)(L + s.up_self) : nullptr;
    a.err = h + JG_HH_ERR;
    const dim3 grid((s.n + JG_BLOCK - 1) / JG_BLOCK), block(JG_BLOCK);
    hipLaunchKernelGGL(k_groups_check_kept, grid, block, 0, e->stream, e->dev, a, gate, h);
    if (open) hipLaunchKernelGGL(k_groups_open_kept, grid, block, 0, e->stream, e->dev, a, gate, h);
    else hipLaunchKernelGGL(k_groups_close_kept, grid, block, 0, e->stream, e->dev, a, gate, h);
    HIPCHK(hipGetLastError());
    e->n_launch += 2;
  }
  HIPCHK(hipEventRecord(o.ev_kernels, e->stream));
  HIPCHK(hipStreamWaitEvent(nd.down, o.ev_kernels, 0));
  HIPCHK(hipMemcpyAsync(o.l_hosting.p, hdr, NODE_HOSTING_LAND, hipMemcpyDeviceToHost, nd.down));
  return JG_OK;
}

// Kept step `o` is being viewed and its outputs have landed: the header words say what each set did - a pass that was gated
// and never queued again did nothing and says so - and become what jg_node_hosting_view hands out.  Before the set's arena
// starts over.
int node_hosting_finish(jg_engine* e, jg_engine::NodeOut& o) {
  (void)e;
  jg_engine::NodeHosting& hs = o.hs;
  jg_node_hosting& v = o.hosting_view;
  v = jg_node_hosting{};
  if (!hs.on) return JG_OK;
  hs.scratch = nullptr;  // (the arena's: gone with it)
  v.attached = 1u, v.state = hs.redone ? (uint32_t)JG_NODE_POLL_REDONE : 0u;
  const uint32_t* const land = (const uint32_t*)o.l_hosting.p;
  for (int open = 0; open < 2; open++) {
    const jg_engine::NodeHostSet& s = open ? hs.open : hs.close;
    if (!s.n) continue;
    const uint32_t* const h = land + (open ? JG_HH_WORDS : 0u);
    if (h[JG_HH_GATE]) return fail(JG_EDEVICE, "internal: a hosted step's pass was gated and not queued again");
    const uint32_t x = h[JG_HH_ERR];
    if (x & (JG_HOST_E_RANGE | JG_HOST_E_ORDER | JG_HOST_E_SLOT)) return fail(JG_EDEVICE, "internal: a hosted step's set failed on the device a check made at entry");
    if (x & JG_HOST_E_DEFER) return fail(JG_EDEVICE, "internal: a hosted step met per-step deferral bits of a listed slot behind the settled step");
    if (x & JG_HOST_E_STATE) v.state |= open ? (uint32_t)JG_NODE_HOSTING_OPEN_REFUSED : (uint32_t)JG_NODE_HOSTING_CLOSE_REFUSED;
    (open ? v.opened : v.closed) = h[JG_HH_WRITTEN];
  }
  return JG_OK;
}

}  // namespace

extern "C" {

int jg_node_hosting_view(jg_engine* e, jg_node_hosting* out) {
  if (!e || !out) return fail(JG_EINVAL, "null argument");
  if (e->router) return fail(JG_EINVAL, "jg_node_hosting_view: a hosted step is a shard's (jg_get_shard)");
  if (e->node.poll_viewed < 0) return fail(JG_EINVAL, "jg_node_hosting_view: no kept step's outbox has been viewed (or a newer step has claimed its set)");
  *out = e->node.sets[e->node.poll_viewed].hosting_view;
  return JG_OK;
}

int jg_engine_open_groups(jg_engine* e, uint64_t now_ms, const jg_group_set* s) { return groups_call(e, true, now_ms, s); }

int jg_engine_close_groups(jg_engine* e, const jg_group_set* s) { return groups_call(e, false, 0, s); }

int jg_engine_list_groups(jg_engine* e, uint32_t which, uint32_t g0, uint32_t n, uint32_t* out, size_t cap, size_t* total) {
  if (!e || !total || (cap && !out)) return fail(JG_EINVAL, "null argument");
  if (which != JG_LIST_VACANT && which != JG_LIST_HOSTED) return fail(JG_EINVAL, "jg_engine_list_groups: unknown `which`");
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_list_groups: slot range out of bounds");
  if (!e->router) return list_shard(e, which, g0, n, 0, out, cap, total);  // (straight into the caller's array)
  // a sharded handle: the shards' answers concatenated in global order (each shard fills what is left of cap)
  const size_t D = shard_count(e);
  std::vector<size_t> tot(D, 0);
  std::vector<std::vector<uint32_t>> part(D);
  int rc = each_shard(e, [&](size_t d) -> int {
    const ShardPart p = shard_part(e, d, g0, n);
    if (!p.n) return JG_OK;
    part[d].resize(std::min<size_t>(cap, p.n));
    return list_shard(shard_at(e, d), which, p.g0, p.n, e->router->lo[d], part[d].data(), part[d].size(), &tot[d]);
  });
  if (rc) return rc;
  size_t all = 0;
  for (size_t d = 0; d < D; d++) {
    const size_t k = std::min<size_t>(std::min<size_t>(tot[d], part[d].size()), cap > all ? cap - all : 0);
    if (k) std::memcpy(out + all, part[d].data(), k * 4);
    all += tot[d];
  }
  *total = all;
  return JG_OK;
}

}  // extern "C"
