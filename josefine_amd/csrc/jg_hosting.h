// jg_hosting.h — gfx950 kernels of jg_engine_open_groups / jg_engine_close_groups / jg_engine_list_groups: which slots of
// an engine host a partition.  A VACANT slot is a group whose sticky fault byte is JG_FAULT_VACANT, so every kernel that
// skips a faulted group ("the reference process is gone") skips it with no change to any hot loop; the one change to the
// shared state machine is that jg_apply does not let a JG_CMD_RESTART / JG_CMD_RECREATE row revive it.
//
//   k_groups_check   one lane per entry of a list or a range: the index's range, strict ascent (the neighbour entry), the
//                    slot's state from its flag word, the own slot; one error word per call, the own slots written -> a mask
//                    (a wave's bits are OR-reduced, and only bits not yet set cost an atomic)
//   k_groups_open    the write pass of an open: jg_restart(empty_store) on a lane loaded from the slot (what a
//                    JG_CMD_RECREATE row does), the own slot first; returns at once when the error word is set
//   k_groups_close   the write pass of a close: the canonical vacant record through jg_store plus the columns a follower's
//                    jg_store leaves alone (packed progress, wide progress, window segments, foreign voters)
//   k_groups_check_kept / k_groups_open_kept / k_groups_close_kept
//                    the same three bodies behind a kept node step (jg_step_node_hosted): one scalar load of the step's
//                    general-row count per workgroup; nonzero, nothing is read or written but the verdict in a header word
//   k_list_count     stream compaction over the flag column (the skeleton of both passes: jg_compact.h), pass 1: per
//                    workgroup the number of matching slots (a 64-bit __ballot and a __popcll per wave and row of 256 slots)
//   k_scan_block_sums (jg_sparse.h) the workgroup counts -> exclusive prefixes and the total
//   k_list_write     pass 2: the same ballots; the first `cap` matching indices ascending (jg_ranked_rows)
//
// The list, the own slots and a range's columns are read and written coalesced; a sparse list's column accesses are a
// scatter (a memory transaction per 4- or 8-byte value) - a control-plane call, not a per-tick one.
#pragma once
#include "jg_compact.h"
#include "jg_device.h"
#include "jg_move.h"    // jg_move_deferred
#include "jg_sparse.h"  // JgScanJob, k_scan_block_sums

#define JG_HOST_E_RANGE 1u   // an index >= G
#define JG_HOST_E_ORDER 2u   // a list that is not strictly ascending
#define JG_HOST_E_STATE 4u   // opening a hosted slot / closing a vacant one
#define JG_HOST_E_SLOT 8u    // self_slots[i] >= R
#define JG_HOST_E_DEFER 16u  // per-step deferral state of a listed slot is pending (internal)
#define JG_LIST_ROWS 16u     // rows of JG_BLOCK slots per workgroup of the list passes
#define JG_LIST_TILE (JG_BLOCK * JG_LIST_ROWS)

struct JgGroupsArgs {
  uint32_t g0, n;        // list == nullptr: shard-local slots [g0, g0 + n)
  const uint32_t* list;  // [n] shard-local indices (device memory)
  const uint8_t* self;   // open: [n] own slots, or nullptr (kept)
  uint32_t open;         // 1: open, 0: close
  uint32_t seq;          // the engine's step number (jg_raise)
  uint64_t now;          // open: the election timer starts here
  uint32_t* err;         // [2] {JG_HOST_E_* bits, own slots an open writes (bit s)}
};

__host__ __device__ __forceinline__ bool jg_flags_vacant(uint32_t f) {
  return ((f & JGF_FAULT_MASK) >> JGF_FAULT_SHIFT) == JG_FAULT_VACANT;
}

__device__ __forceinline__ uint32_t jg_wave_or(uint32_t v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v |= __shfl_xor(v, off, 64);
  return v;
}

// this lane's entry of a set, checked - the body of k_groups_check and k_groups_check_kept (every lane of a workgroup calls
// it; the arguments by value: by reference the compiler schedules k_groups_check differently from the kernel it was)
__device__ __forceinline__ void jg_groups_check_entry(JgDev d, JgGroupsArgs a) {
  const uint32_t i = blockIdx.x * JG_BLOCK + threadIdx.x;
  uint32_t e = 0, slots = 0;
  if (i < a.n) {
    const uint32_t g = a.list ? a.list[i] : a.g0 + i;
    if (a.list && i > 0 && a.list[i - 1] >= g) e |= JG_HOST_E_ORDER;
    const uint32_t s = a.self ? a.self[i] : 0u;
    if (s >= d.R) e |= JG_HOST_E_SLOT;
    if (g >= d.G) {
      e |= JG_HOST_E_RANGE;
    } else {
      const uint32_t f = d.flags[g];
      if (jg_flags_vacant(f) != (a.open != 0)) e |= JG_HOST_E_STATE;
      if (jg_move_deferred(d, g)) e |= JG_HOST_E_DEFER;
      if (a.open && a.self && s < d.R) slots = 1u << s;
      else if (a.open) slots = 1u << ((f & JGF_SELF_MASK) >> JGF_SELF_SHIFT);
    }
  }
  // (every lane reaches the reductions)
  e = jg_wave_or(e);
  slots = jg_wave_or(slots);
  // (an atomic only where it adds a bit: one per wave on one address serialised a 16 M-slot open to 3 ms)
  if ((threadIdx.x & 63u) == 0) {
    if (e && (*(volatile uint32_t*)a.err & e) != e) atomicOr(a.err, e);
    if (slots && (*(volatile uint32_t*)(a.err + 1) & slots) != slots) atomicOr(a.err + 1, slots);
  }
}

__global__ __launch_bounds__(JG_BLOCK) void k_groups_check(JgDev d, JgGroupsArgs a) {
  jg_groups_check_entry(d, a);
}

// this lane's entry of an open, written - the body of k_groups_open and k_groups_open_kept
__device__ __forceinline__ void jg_groups_open_entry(const JgDev& d, const JgGroupsArgs& a) {
  if (*(volatile uint32_t*)a.err) return;  // refused: nothing is written
  const uint32_t i = blockIdx.x * JG_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t g = a.list ? a.list[i] : a.g0 + i;
  JgLane L;
  jg_load(d, L, g);  // the vacant record: a follower, genesis only, the carried draw count
  L.now = a.now, L.seq = a.seq;
  L.mp = L.mend = nullptr, L.fp = L.fend = nullptr;
  if (a.self) L.flags = (L.flags & ~JGF_SELF_MASK) | ((uint32_t)a.self[i] << JGF_SELF_SHIFT);
  jg_restart(d, L, true);  // what a JG_CMD_RECREATE row does at now (it clears the fault byte)
  jg_store<false>(d, L);
}

__global__ __launch_bounds__(JG_BLOCK) void k_groups_open(JgDev d, JgGroupsArgs a) {
  jg_groups_open_entry(d, a);
}

// this lane's entry of a close, written - the body of k_groups_close and k_groups_close_kept
__device__ __forceinline__ void jg_groups_close_entry(const JgDev& d, const JgGroupsArgs& a) {
  if (*(volatile uint32_t*)a.err) return;
  const uint32_t i = blockIdx.x * JG_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t g = a.list ? a.list[i] : a.g0 + i;
  const uint32_t f = d.flags[g];
  const uint32_t draws = d.cold.t[g].w;  // kept: a slot closed and reopened never reuses a timeout draw
  JgLane L;
  L.g = g;
  L.term = 0;
  L.commit = L.head = 0;  // Chain::new on an empty directory: genesis only
  L.id_gen = 1;
  L.run_hi = 0;
  L.heartbeat_time = 0;
  L.election_time = 0;
  L.election_timeout = 0;
  L.rng_draws = draws;
  L.voted_for = L.leader_id = L.queued = L.votes = 0;
  L.mword = 0, L.mbase = 0;
  L.flags = JG_ROLE_FOLLOWER | (f & JGF_SELF_MASK) | (JG_FAULT_VACANT << JGF_FAULT_SHIFT);
  jg_store<false>(d, L);  // (a follower: RUN and FAST form, the absolute commit column)
  const size_t G = d.G;
  d.mlag[g] = 0;  // every progress head 0, Probe (the REPL bits are clear)
  for (uint32_t r = 0; r < d.R; r++) d.match_wide[(size_t)r * G + g] = 0;
  for (uint32_t w = 0; w < JG_CHAIN_WINDOW; w++) {
    d.win_lo[(size_t)w * G + g] = 0;
    d.win_hi[(size_t)w * G + g] = 0;
    d.win_next[(size_t)w * G + g] = 0;
  }
  for (uint32_t v = 0; v < JG_FOREIGN_VOTERS; v++) d.fvote_id[(size_t)v * G + g] = 0;
}

__global__ __launch_bounds__(JG_BLOCK) void k_groups_close(JgDev d, JgGroupsArgs a) {
  jg_groups_close_entry(d, a);
}

// Hosting behind a kept node step (jg_step_node_hosted): per set four header words, a.err == hdr + JG_HH_ERR.  `gate`: the
// step's general-row count on the device, or null.  Nonzero - the step is completed by a catch-up pass, the columns are not
// the settled state's yet - and no lane loads or stores anything: lane 0 of workgroup 0 leaves the verdict in hdr[JG_HH_GATE]
// and the three launches are queued once more, ungated, behind the catch-up pass.  Zero or null: the plain kernels' bodies,
// the write pass returning where the check pass raised the error word - no host read sits between the two.
#define JG_HH_GATE 0u     // the gate's verdict: the step's general-path rows as the check pass saw them
#define JG_HH_ERR 1u      // JG_HOST_E_* bits (JgGroupsArgs::err[0])
#define JG_HH_SLOTS 2u    // the own slots an open writes (JgGroupsArgs::err[1])
#define JG_HH_WRITTEN 3u  // the slots the write pass wrote: n, or 0 (refused, or gated)
#define JG_HH_WORDS 4u

__global__ __launch_bounds__(JG_BLOCK) void k_groups_check_kept(JgDev d, JgGroupsArgs a, const uint32_t* gate, uint32_t* hdr) {
  const uint32_t gated = gate ? *gate : 0u;  // (uniform: one scalar load per workgroup)
  if (blockIdx.x == 0 && threadIdx.x == 0) hdr[JG_HH_GATE] = gated;
  if (gated) return;
  jg_groups_check_entry(d, a);
}

__global__ __launch_bounds__(JG_BLOCK) void k_groups_open_kept(JgDev d, JgGroupsArgs a, const uint32_t* gate, uint32_t* hdr) {
  const uint32_t gated = gate ? *gate : 0u;
  if (gated) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) hdr[JG_HH_WRITTEN] = *(volatile uint32_t*)a.err ? 0u : a.n;
  jg_groups_open_entry(d, a);
}

__global__ __launch_bounds__(JG_BLOCK) void k_groups_close_kept(JgDev d, JgGroupsArgs a, const uint32_t* gate, uint32_t* hdr) {
  const uint32_t gated = gate ? *gate : 0u;
  if (gated) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) hdr[JG_HH_WRITTEN] = *(volatile uint32_t*)a.err ? 0u : a.n;
  jg_groups_close_entry(d, a);
}

struct JgListArgs {
  uint32_t g0, n;   // shard-local slots [g0, g0 + n)
  uint32_t which;   // JG_LIST_VACANT / JG_LIST_HOSTED
  uint32_t add;     // added to every index written (a shard's first global slot)
  uint64_t* bsum;   // [tiles] the workgroup counts, then (k_scan_block_sums) their exclusive prefixes
  uint32_t* out;    // [cap] (device)
  uint64_t cap;
};

// the 16 ballots of a workgroup's rows: bit l of m[k] = slot t0 + k * JG_BLOCK + (wave * 64 + l) matches
__device__ __forceinline__ void jg_list_ballots(const JgDev& d, const JgListArgs& a, uint64_t* m) {
  const uint32_t t0 = blockIdx.x * JG_LIST_TILE + threadIdx.x;
  uint32_t f[JG_LIST_ROWS];
#pragma unroll
  for (uint32_t k = 0; k < JG_LIST_ROWS; k++) {  // (the loads first: sixteen in flight per lane)
    const uint32_t i = t0 + k * JG_BLOCK;
    f[k] = i < a.n ? d.flags[a.g0 + i] : 0u;
  }
#pragma unroll
  for (uint32_t k = 0; k < JG_LIST_ROWS; k++) {
    const uint32_t i = t0 + k * JG_BLOCK;
    m[k] = __ballot(i < a.n && jg_flags_vacant(f[k]) == (a.which == JG_LIST_VACANT));
  }
}

__global__ __launch_bounds__(JG_BLOCK) void k_list_count(JgDev d, JgListArgs a) {
  uint64_t m[JG_LIST_ROWS];
  jg_list_ballots(d, a, m);
  uint32_t c = 0;
#pragma unroll
  for (uint32_t k = 0; k < JG_LIST_ROWS; k++) c += __popcll(m[k]);
  const uint32_t t = jg_tile_count(c);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = t;
}

__global__ __launch_bounds__(JG_BLOCK) void k_list_write(JgDev d, JgListArgs a) {
  const uint64_t base = a.bsum[blockIdx.x];
  if (base >= a.cap) return;  // (uniform over the workgroup) its matches are all beyond cap
  uint64_t m[JG_LIST_ROWS];
  jg_list_ballots(d, a, m);
  const uint32_t t0 = blockIdx.x * JG_LIST_TILE + threadIdx.x;
  jg_ranked_rows<JG_LIST_ROWS>(m, base, a.cap, [&](uint32_t k, uint64_t pos) { a.out[pos] = a.add + a.g0 + t0 + k * JG_BLOCK; });
}
