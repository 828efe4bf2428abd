// jg_watch.h — gfx950 kernels of jg_engine_watch_leaders / jg_engine_census: what changed leader, and what is.
//
// The LEADERSHIP VIEW of a slot is a function of three things already in HBM - the flag word, the term column and the
// 16-byte cold_v record (the leader id a follower knows) - and of nothing else (jg_lead_view).  A watch compares it with a
// SHADOW: the view last reported, 16 bytes per slot {term, leader id, role | state << 8 | fault << 16}, allocated at the
// engine's first watch.  The meta word is stored XOR the vacant view's, so the zero-filled allocation IS "every slot was
// last reported vacant".
//
//   k_watch_count      stream compaction over "view != shadow" (the skeleton of both passes: jg_compact.h), pass 1: per
//                      workgroup the number of slots that differ (a 64-bit __ballot and a __popcll per wave and row of
//                      256 slots); 44 bytes read per slot
//   k_scan_block_sums  (jg_sparse.h) the workgroup counts -> exclusive prefixes and the total
//   k_watch_write      pass 2: a workgroup with nothing to report or wholly beyond `cap` returns at once; else the same
//                      ballots, the first `cap` rows ascending (jg_ranked_rows), and - unless peeking - the shadow of
//                      exactly those slots
//   k_census           one pass of 1-bit predicates counted by ballots (one wave-uniform add per field and row), the term
//                      maximum and the leaders' head - commit by __shfl_down; one partial record per workgroup
//                      (jg_block_words)
//   k_census_sum       the partial records -> the census (jg_parts_reduce: one workgroup; no atomics anywhere)
//
// Nothing here writes a column of the state machine: the only stores are the scratch, the rows and the shadow.
#pragma once
#include "jg_compact.h"
#include "jg_device.h"
#include "jg_hosting.h"  // jg_flags_vacant
#include "jg_read.h"     // jg_read_commit
#include "jg_sparse.h"   // JgScanJob, k_scan_block_sums

#define JG_WATCH_ROWS 4u  // rows of JG_BLOCK slots per workgroup of the watch passes (44 bytes in flight per lane and row)
#define JG_WATCH_TILE (JG_BLOCK * JG_WATCH_ROWS)
#define JG_CENSUS_ROWS 16u  // ... of the census pass: one partial record per 4096 slots
#define JG_CENSUS_TILE (JG_BLOCK * JG_CENSUS_ROWS)
// the meta word of the vacant view: what the shadow's meta word is stored XOR
#define JG_WATCH_VACANT_META (((uint32_t)JG_LEAD_VACANT << 8) | ((uint32_t)JG_FAULT_VACANT << 16))

// a census as the words the kernels add up: the fields of jg_census in order
#define JG_CENSUS_LED_BY 8u
#define JG_CENSUS_MAX_TERM (JG_CENSUS_LED_BY + JG_MAX_REPLICAS + 1u)
#define JG_CENSUS_UNCOMMITTED (JG_CENSUS_MAX_TERM + 1u)
#define JG_CENSUS_WORDS (JG_CENSUS_UNCOMMITTED + 1u)
static_assert(sizeof(jg_census) == JG_CENSUS_WORDS * 8, "jg_census is the census words in order");
static_assert(sizeof(jg_leader_row) == 24, "jg_leader_row is three 8-byte pieces");

// the view as the shadow holds it
struct JgLeadView {
  uint64_t term;
  uint32_t leader_id;
  uint32_t meta;  // role | state << 8 | fault << 16
};

__device__ __forceinline__ JgLeadView jg_lead_view(const JgDev& d, uint32_t f, uint64_t term, uint32_t follower_leader) {
  JgLeadView v;
  const uint32_t fault = (f & JGF_FAULT_MASK) >> JGF_FAULT_SHIFT, role = f & JGF_ROLE_MASK;
  if (fault == JG_FAULT_VACANT) {
    v.term = 0, v.leader_id = 0, v.meta = JG_WATCH_VACANT_META;
    return v;
  }
  uint32_t state = fault ? (uint32_t)JG_LEAD_FAULTED : 0u;
  v.term = term;
  v.leader_id = 0;
  if (role == JG_ROLE_LEADER) {
    v.leader_id = d.node_ids[(f & JGF_SELF_MASK) >> JGF_SELF_SHIFT];
    state |= JG_LEAD_KNOWN | JG_LEAD_SELF;
  } else if (role == JG_ROLE_FOLLOWER && (f & JGF_HAS_LEADER)) {
    v.leader_id = follower_leader;
    state |= JG_LEAD_KNOWN;
  }
  v.meta = role | (state << 8) | (fault << 16);
  return v;
}
// the view as the shadow's 16 bytes, and "the shadow sh is not the view v"
__device__ __forceinline__ uint4 jg_lead_shadow(const JgLeadView& v) {
  return make_uint4((uint32_t)v.term, (uint32_t)(v.term >> 32), v.leader_id, v.meta ^ JG_WATCH_VACANT_META);
}
__device__ __forceinline__ bool jg_lead_differs(const uint4& sh, const JgLeadView& v) {
  return sh.x != (uint32_t)v.term || sh.y != (uint32_t)(v.term >> 32) || sh.z != v.leader_id || sh.w != (v.meta ^ JG_WATCH_VACANT_META);
}

// the peek a pass acts on: the call's own, or the gate's verdict - ONE scalar load per workgroup (the pointer and the word are
// uniform), taken behind the early return of a quiet workgroup, never inside the walk over the slots
__device__ __forceinline__ uint32_t jg_gated_peek(uint32_t peek, const uint32_t* gate) { return peek | (gate ? *gate : 0u); }

struct JgWatchArgs {
  uint32_t g0, n;    // shard-local slots [g0, g0 + n)
  uint32_t add;      // added to every group written (a shard's first global slot)
  uint32_t peek;     // 1: the shadow is left alone
  uint4* shadow;     // [G]
  uint32_t* cnt;     // [tiles] the workgroup counts
  uint64_t* bsum;    // [tiles] the same, then (k_scan_block_sums) their exclusive prefixes
  jg_leader_row* out;  // [cap] (device)
  uint64_t cap;
  const uint32_t* gate;  // null, or a device word: nonzero = behave as under peek (a polled node step whose rows took the general path)
};

// a workgroup's rows: v[k] the view of slot t0 + k * JG_BLOCK, f[k] its flag word, bit l of m[k] = the slot of lane l of
// this wave differs from its shadow.  (the loads first: four a row, sixteen in flight per lane)
__device__ __forceinline__ void jg_watch_ballots(const JgDev& d, const JgWatchArgs& a, JgLeadView* v, uint32_t* f, uint64_t* m) {
  const uint32_t t0 = blockIdx.x * JG_WATCH_TILE + threadIdx.x;
  uint64_t term[JG_WATCH_ROWS];
  uint4 cold[JG_WATCH_ROWS], sh[JG_WATCH_ROWS];
#pragma unroll
  for (uint32_t k = 0; k < JG_WATCH_ROWS; k++) {
    const uint32_t i = t0 + k * JG_BLOCK;
    const bool in = i < a.n;
    const uint32_t g = a.g0 + (in ? i : 0u);
    f[k] = in ? d.flags[g] : 0u;
    term[k] = in ? d.term[g] : 0ull;
    cold[k] = in ? d.cold.v[g] : make_uint4(0, 0, 0, 0);
    sh[k] = in ? a.shadow[g] : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (uint32_t k = 0; k < JG_WATCH_ROWS; k++) {
    const uint32_t i = t0 + k * JG_BLOCK;
    v[k] = jg_lead_view(d, f[k], term[k], cold[k].y);
    m[k] = __ballot(i < a.n && jg_lead_differs(sh[k], v[k]));
  }
}

__global__ __launch_bounds__(JG_BLOCK) void k_watch_count(JgDev d, JgWatchArgs a) {
  JgLeadView v[JG_WATCH_ROWS];
  uint32_t f[JG_WATCH_ROWS];
  uint64_t m[JG_WATCH_ROWS];
  jg_watch_ballots(d, a, v, f, m);
  uint32_t c = 0;
#pragma unroll
  for (uint32_t k = 0; k < JG_WATCH_ROWS; k++) c += __popcll(m[k]);
  const uint32_t t = jg_tile_count(c);
  if (threadIdx.x == 0) a.cnt[blockIdx.x] = t, a.bsum[blockIdx.x] = t;
}

__global__ __launch_bounds__(JG_BLOCK) void k_watch_write(JgDev d, JgWatchArgs a) {
  const uint64_t base = a.bsum[blockIdx.x];
  // (uniform over the workgroup) nothing differs here - the quiet engine's every workgroup - or it is all beyond cap
  if (a.cnt[blockIdx.x] == 0 || base >= a.cap) return;
  JgLeadView v[JG_WATCH_ROWS];
  uint32_t f[JG_WATCH_ROWS];
  uint64_t m[JG_WATCH_ROWS];
  jg_watch_ballots(d, a, v, f, m);
  const uint32_t peek = jg_gated_peek(a.peek, a.gate);
  const uint32_t t0 = blockIdx.x * JG_WATCH_TILE + threadIdx.x;
  uint64_t* out64 = (uint64_t*)a.out;
  jg_ranked_rows<JG_WATCH_ROWS>(m, base, a.cap, [&](uint32_t k, uint64_t pos) {
    const uint32_t g = a.g0 + t0 + k * JG_BLOCK;
    const uint32_t self = (f[k] & JGF_SELF_MASK) >> JGF_SELF_SHIFT;
    // the row as three 8-byte pieces: {group, leader_id} {term} {role, state, fault, self_slot, reserved}
    out64[pos * 3 + 0] = (uint64_t)(a.add + g) | (uint64_t)v[k].leader_id << 32;
    out64[pos * 3 + 1] = v[k].term;
    out64[pos * 3 + 2] = (uint64_t)(v[k].meta | self << 24);
    if (!peek) a.shadow[g] = jg_lead_shadow(v[k]);
  });
}

struct JgCensusArgs {
  uint32_t g0, n;   // shard-local slots [g0, g0 + n)
  uint32_t tiles;   // workgroups of k_census
  uint32_t pad;
  uint64_t* part;   // [tiles][JG_CENSUS_WORDS] the workgroups' partial records
  uint64_t* out;    // [JG_CENSUS_WORDS]
};

__global__ __launch_bounds__(JG_BLOCK) void k_census(JgDev d, JgCensusArgs a) {
  const uint32_t t0 = blockIdx.x * JG_CENSUS_TILE + threadIdx.x;
  uint32_t c[JG_CENSUS_MAX_TERM];  // the counted fields: wave-uniform (every lane adds the same popcount)
#pragma unroll
  for (uint32_t x = 0; x < JG_CENSUS_MAX_TERM; x++) c[x] = 0;
  uint64_t max_term = 0, uncommitted = 0;  // per lane
  for (uint32_t k0 = 0; k0 < JG_CENSUS_ROWS; k0 += 4) {
    uint32_t f[4];
    uint64_t term[4];
    uint4 cold[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {  // (the loads first)
      const uint32_t i = t0 + (k0 + k) * JG_BLOCK;
      const bool in = i < a.n;
      const uint32_t g = a.g0 + (in ? i : 0u);
      f[k] = in ? d.flags[g] : (uint32_t)JG_FAULT_VACANT << JGF_FAULT_SHIFT;
      term[k] = in ? d.term[g] : 0ull;
      cold[k] = in ? d.cold.v[g] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      const uint32_t i = t0 + (k0 + k) * JG_BLOCK;
      const bool in = i < a.n;
      const uint32_t g = a.g0 + (in ? i : 0u);
      const JgLeadView v = jg_lead_view(d, f[k], term[k], cold[k].y);
      const uint32_t fault = (v.meta >> 16) & 0xffu, role = v.meta & 0xffu, state = (v.meta >> 8) & 0xffu;
      const bool hosted = in && fault != JG_FAULT_VACANT, healthy = hosted && fault == 0;
      const bool known = healthy && (state & JG_LEAD_KNOWN);
      c[0] += __popcll(__ballot(hosted));
      c[1] += __popcll(__ballot(in && !hosted));
      c[2] += __popcll(__ballot(hosted && fault >= 1u && fault < 128u));
      c[3] += __popcll(__ballot(hosted && fault >= 128u));
      c[4] += __popcll(__ballot(healthy && role == JG_ROLE_FOLLOWER));
      c[5] += __popcll(__ballot(healthy && role == JG_ROLE_CANDIDATE));
      c[6] += __popcll(__ballot(healthy && role == JG_ROLE_LEADER));
      c[7] += __popcll(__ballot(healthy && !known));
      bool member = false;
#pragma unroll
      for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++) {
        const bool is = known && !member && r < d.R && v.leader_id == d.node_ids[r];
        c[JG_CENSUS_LED_BY + r] += __popcll(__ballot(is));
        member = member || is;
      }
      c[JG_CENSUS_LED_BY + JG_MAX_REPLICAS] += __popcll(__ballot(known && !member));
      if (hosted && v.term > max_term) max_term = v.term;
      if (healthy && role == JG_ROLE_LEADER) uncommitted += d.head[g] - jg_read_commit(d, g, f[k]);
    }
  }
  uint64_t vals[JG_CENSUS_WORDS];
#pragma unroll
  for (uint32_t x = 0; x < JG_CENSUS_MAX_TERM; x++) vals[x] = c[x];
  vals[JG_CENSUS_MAX_TERM] = jg_wave_max64(max_term);
  vals[JG_CENSUS_UNCOMMITTED] = jg_wave_sum64(uncommitted);
  jg_block_words<JG_CENSUS_WORDS>(vals, [](uint32_t x) { return x == JG_CENSUS_MAX_TERM; }, a.part);
}

__global__ __launch_bounds__(JG_BLOCK) void k_census_sum(JgCensusArgs a) {
  jg_parts_reduce<JG_CENSUS_WORDS>(a.part, a.tiles, a.out, [](uint32_t x) { return x == JG_CENSUS_MAX_TERM; });
}
