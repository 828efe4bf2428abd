// jg_lookup.h — gfx950 kernels of jg_engine_lookup_groups: the state of a LIST of slots, one 80-byte row per entry in the
// order asked, every jg_read_state field of the slot plus its leadership view (jg_lead_view), and optionally the leader's
// R progress heads.
//
// A list names slots in the caller's order - unsorted, with repeats - so an entry's columns are a gather: about ten
// independent 64-byte sectors (the flag word, six 8-byte columns, the packed progress word, the two 16-byte cold records),
// of which the row uses 70 bytes.  The kernel is bound by round trips, not bytes: every unconditional load of an entry is
// issued before the first use (ONE trip to memory per entry, as the dense kernels' "one round trip"), and only the wide
// progress column - an escaped lag field, rare - is loaded under a branch.  The range form is the same kernel with
// g = g0 + i: its loads and stores coalesce.
//
//   k_lookup<R>      one lane per entry: the loads, the decode with the helpers jg_read_state and the feeds use
//                    (jg_lag_field, jg_lag_wide, jg_lag_base_is_run_hi, jg_read_commit, jg_lead_view), the row as five
//                    16-byte stores - consecutive lanes, consecutive rows - and, asked for, R 8-byte progress heads.  An
//                    index >= G (a device list: a host list is checked on the host) raises the call's error word with a
//                    plain store and touches no column
//   k_lookup_kept<R> the same body behind a kept node step (jg_step_node_looked): one scalar load of the step's general-row
//                    count per workgroup; nonzero, no row is written and the verdict is left in a header word
//   k_lookup_check   a device list longer than one staging piece: the bounds of every entry before the first piece is
//                    made, so that nothing reaches the caller from a list that is refused
//
// No atomics, no LDS, no scratch.  Nothing here writes a column of the state machine: the only stores are the rows, the
// progress heads and the error word.
#pragma once
#include "jg_device.h"
#include "jg_read.h"   // jg_read_commit
#include "jg_watch.h"  // jg_lead_view

static_assert(sizeof(jg_group_state) == 80, "jg_group_state is five 16-byte pieces");

typedef uint32_t jg_u32x4 __attribute__((ext_vector_type(4)));  // a 16-byte piece of a row: one store

struct JgLookupArgs {
  uint32_t g0, n;        // list == nullptr: shard-local slots g0 .. g0 + n - 1
  const uint32_t* list;  // [n] shard-local indices (device memory), any order, repeats allowed
  uint32_t add;          // added to every group written (a shard's first global slot)
  uint32_t pad;
  uint4* out;            // [n] rows (device, 16-byte aligned)
  uint64_t* match;       // [n][R] progress heads, or nullptr
  uint32_t* err;         // [1] set to 1 by an index >= G
};

// entry i of the list: the loads, the decode, the row and (asked for) the progress heads - the body of both kernels
template <int R>
__device__ __forceinline__ void jg_lookup_entry(const JgDev& d, const JgLookupArgs& a, uint32_t i) {
  if (i >= a.n) return;
  const uint32_t g = a.list ? a.list[i] : a.g0 + i;  // (uniform over the launch)
  if (g >= d.G) {
    *a.err = 1u;  // (every lane that stores, stores the same word)
    return;
  }
  // one round trip: the ten unconditional loads of the entry, back to back
  const uint32_t f = d.flags[g];
  const uint64_t term = d.term[g], head = d.head[g], commit = d.commit[g], w = d.mlag[g], run_hi = d.run_hi[g], id_gen = d.id_gen[g],
                 hbt = d.heartbeat_time[g];
  const uint4 ct = d.cold.t[g], cv = d.cold.v[g];
  const uint32_t role = f & JGF_ROLE_MASK, fault = (f & JGF_FAULT_MASK) >> JGF_FAULT_SHIFT, self = (f & JGF_SELF_MASK) >> JGF_SELF_SHIFT;
  const bool leader = role == JG_ROLE_LEADER, knows = role == JG_ROLE_FOLLOWER && (f & JGF_HAS_LEADER);
  const JgLeadView v = jg_lead_view(d, f, term, cv.y);
  const uint64_t commit_now = jg_read_commit(d, g, f);  // (its loads are the ones above: nothing was stored since)
  // (the loads stay up there: without an unconditional use the compiler sinks a load behind the branch that consumes it -
  // a second, dependent trip.  Placed behind the helpers, whose loads of the same words fold into the ones above)
  asm volatile("" ::"v"(f), "v"(term), "v"(head), "v"(commit), "v"(w), "v"(run_hi), "v"(id_gen), "v"(hbt));
  asm volatile("" ::"v"(ct.x), "v"(ct.y), "v"(ct.z), "v"(cv.x), "v"(cv.y), "v"(cv.z), "v"(cv.w));
  const uint64_t idg = (f & JGF_FAST) ? head + 1 : id_gen;
  const uint64_t hb = leader ? hbt : 0ull;
  const uint32_t voted_for = (f & JGF_VOTED) ? cv.x : 0u, leader_id = knows ? cv.y : 0u;
  const uint32_t votes = role == JG_ROLE_CANDIDATE ? cv.w : 0u;
  const uint32_t repl = leader ? (f & JGF_REPL_MASK) >> JGF_REPL_SHIFT : 0u;
  const uint32_t has = ((f & JGF_VOTED) ? 1u : 0u) | (knows ? 2u : 0u);
  const uint32_t b0 = role | ((v.meta >> 8) & 0xffu) << 8 | fault << 16 | self << 24;
  const uint32_t b1 = repl | (votes & 0xffu) << 8 | ((votes >> 8) & 0xffu) << 16 | has << 24;
  auto lo = [](uint64_t x) { return (uint32_t)x; };
  auto hi = [](uint64_t x) { return (uint32_t)(x >> 32); };
  // the row: {group, known_leader, term} {head, commit} {id_gen, election_time} {heartbeat_time, voted_for, leader_id}
  // {election_timeout, queued_reqs, role | state | fault | self_slot, repl_state | vote_seen | vote_granted | has}
  jg_u32x4* o = (jg_u32x4*)(a.out + (size_t)i * 5);
  o[0] = jg_u32x4{a.add + g, v.leader_id, lo(term), hi(term)};
  o[1] = jg_u32x4{lo(head), hi(head), lo(commit_now), hi(commit_now)};
  o[2] = jg_u32x4{lo(idg), hi(idg), ct.x, ct.y};
  o[3] = jg_u32x4{lo(hb), hi(hb), voted_for, leader_id};
  o[4] = jg_u32x4{ct.z, cv.z, b0, b1};
  if (a.match) {  // (uniform over the launch) JG_FIELD_MATCH of every member: 0 for a slot that is not a leader
    const uint64_t base = jg_lag_base_is_run_hi(f) ? run_hi : head;
    uint64_t* m = a.match + (size_t)i * R;
#pragma unroll
    for (uint32_t r = 0; r < (uint32_t)R; r++) {
      const uint64_t field = jg_lag_field(w, r, R);
      m[r] = !leader ? 0ull : jg_lag_wide(field, R) ? d.match_wide[(size_t)r * d.G + g] : base - field;
    }
  }
}

template <int R>
__global__ __launch_bounds__(JG_BLOCK) void k_lookup(JgDev d, JgLookupArgs a) {
  jg_lookup_entry<R>(d, a, blockIdx.x * JG_BLOCK + threadIdx.x);
}

// the lookup behind a kept node step (jg_step_node_looked).  `gate`: the step's general-row count on the device, or null.
// Nonzero - the step is completed by a catch-up pass, the columns are not the settled state's yet - and the pass writes no
// row: it leaves the verdict in hdr[JG_LH_GATE] and is queued once more, ungated, behind the catch-up pass.  Zero or null:
// k_lookup, and a verdict of 0.
#define JG_LH_GATE 0u   // the gate's verdict: the step's general-path rows as this pass saw them
#define JG_LH_ERR 1u    // k_lookup's error word (a host list is checked on the host: stays 0)
#define JG_LH_WORDS 2u

template <int R>
__global__ __launch_bounds__(JG_BLOCK) void k_lookup_kept(JgDev d, JgLookupArgs a, const uint32_t* gate, uint32_t* hdr) {
  const uint32_t gated = gate ? *gate : 0u;  // (uniform: one scalar load per workgroup)
  if (blockIdx.x == 0 && threadIdx.x == 0) hdr[JG_LH_GATE] = gated;
  if (gated) return;
  jg_lookup_entry<R>(d, a, blockIdx.x * JG_BLOCK + threadIdx.x);
}

__global__ __launch_bounds__(JG_BLOCK) void k_lookup_check(uint32_t G, const uint32_t* list, uint64_t n, uint32_t* err) {
  for (uint64_t i = (uint64_t)blockIdx.x * JG_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * JG_BLOCK)
    if (list[i] >= G) *err = 1u;
}
