// jg_isr.h — gfx950 kernels of jg_engine_watch_replicas / jg_engine_replication_census: which replicas of the partitions
// this engine leads are in sync, and which member is falling behind.
//
// The REPLICATION VIEW of a slot that leads (role leader, fault 0) is the set of members whose lag `head - match` is within
// a threshold, the own slot always; of any other slot it is 0.  A leader's R progress heads are the lag fields of ONE
// 64-bit word (d.mlag, jg_device.h), so in the common case - no field an escape, the lags relative to the head - the whole
// set is arithmetic on that word: a watch decides "did the set of this slot change?" from the flag word, mlag[g] and the
// SHADOW word, 16 bytes per slot.  The shadow is 4 bytes per slot {isr | LEADS << 8} as last reported, allocated at the
// engine's first watch; zero-filled it says "not leading, empty set".  Membership is hysteretic AGAINST the shadow: a member
// the shadow holds stays while its lag is <= leave_lag, any other joins at lag <= join_lag.
//
//   k_isr_count        stream compaction over "view != shadow" (the skeleton of both passes: jg_compact.h), pass 1: per
//                      workgroup the number of slots that differ (a 64-bit __ballot and a __popcll per wave and row of
//                      256 slots); 16 bytes read per slot, the rare fields (an escape, a base that is run_hi) decoded
//                      exactly under a branch
//   k_scan_block_sums  (jg_sparse.h) the workgroup counts -> exclusive prefixes and the total
//   k_isr_write        pass 2: a workgroup with nothing to report or wholly beyond `cap` returns after two loads; else the
//                      same ballots and jg_isr_write_rows (k_isrc_write's too): the head of the slots that differ, the
//                      first `cap` rows ascending as three 8-byte stores, and - unless peeking - the shadow word of
//                      exactly those slots
//   k_repl_census      one threshold, no shadow: the 1-bit predicates counted by ballots (one wave-uniform add per field
//                      and row), the per-member lag maxima and sums and the largest head - commit by __shfl_down; a
//                      workgroup strides over the tiles, so there are at most JG_REPL_CENSUS_PARTS partial records
//                      (jg_block_words)
//   k_repl_census_sum  the partial records -> the census (jg_parts_reduce: one workgroup; no atomics anywhere)
//
// Nothing here writes a column of the state machine: the only stores are the scratch, the rows and the shadow.
#pragma once
#include "jg_device.h"
#include "jg_read.h"    // jg_read_commit
#include "jg_sparse.h"  // JgScanJob, k_scan_block_sums
#include "jg_watch.h"   // jg_gated_peek (and jg_compact.h)

#define JG_ISR_ROWS 4u  // rows of JG_BLOCK slots per workgroup of the watch passes (16 bytes in flight per lane and row)
#define JG_ISR_TILE (JG_BLOCK * JG_ISR_ROWS)
#define JG_ISR_SHADOW_LEADS 0x100u  // the shadow word: isr | this where the slot led
#define JG_REPL_CENSUS_ROWS 4u      // rows per tile of the census pass
#define JG_REPL_CENSUS_TILE (JG_BLOCK * JG_REPL_CENSUS_ROWS)
// the most workgroups - partial records - of the census pass: four a CU on 256 CUs.  A workgroup takes the tiles
// b, b + grid, ..., so k_repl_census_sum walks at most this many records whatever the engine's size (k_census_sum walks
// 4096 at 16 M slots: 61 us) and no second level is needed
#define JG_REPL_CENSUS_PARTS 1024u

// a replication census as the words the kernels reduce: the fields of jg_repl_census in order
#define JG_RC_OUT_OF_SYNC 4u
#define JG_RC_MAX_LAG (JG_RC_OUT_OF_SYNC + JG_MAX_REPLICAS)
#define JG_RC_SUM_LAG (JG_RC_MAX_LAG + JG_MAX_REPLICAS)
#define JG_RC_MAX_UNCOMMITTED (JG_RC_SUM_LAG + JG_MAX_REPLICAS)
#define JG_RC_WORDS (JG_RC_MAX_UNCOMMITTED + 1u)
static_assert(sizeof(jg_repl_census) == JG_RC_WORDS * 8, "jg_repl_census is the census words in order");
static_assert(sizeof(jg_isr_row) == 24, "jg_isr_row is three 8-byte pieces");
__host__ __device__ __forceinline__ bool jg_rc_is_max(uint32_t x) {
  return (x >= JG_RC_MAX_LAG && x < JG_RC_SUM_LAG) || x == JG_RC_MAX_UNCOMMITTED;
}

// a slot leads for the feed: role leader, fault 0 (a vacant slot carries fault 255)
__device__ __forceinline__ bool jg_isr_leads(uint32_t f) { return (f & (JGF_ROLE_MASK | JGF_FAULT_MASK)) == JG_ROLE_LEADER; }

// the lag of member r of a leading slot, decoded as jg_read_state decodes MATCH (the wide column where the field is an
// escape, else base - field), saturating: a progress head above the chain head counts as caught up
__device__ __forceinline__ uint64_t jg_isr_lag_exact(const JgDev& d, uint32_t g, uint64_t field, uint32_t r, uint64_t base, uint64_t head) {
  const uint64_t match = jg_lag_wide(field, d.R) ? d.match_wide[(size_t)r * d.G + g] : base - field;
  return head > match ? head - match : 0ull;
}

// The in-sync set of slot g as the shadow holds it (isr | LEADS, 0 for a slot that does not lead) from its flag word f,
// its packed word w and its shadow word sh.  leave / join: the thresholds; leave32 / join32: the same clamped to 32 bits
// for the fields of the common case.
__device__ __forceinline__ uint32_t jg_isr_word(const JgDev& d, uint64_t leave, uint64_t join, uint32_t leave32, uint32_t join32, uint32_t g,
                                                uint32_t f, uint64_t w, uint32_t sh) {
  if (!jg_isr_leads(f)) return 0u;
  const uint32_t R = d.R, self = (f & JGF_SELF_MASK) >> JGF_SELF_SHIFT;
  const uint32_t was = (sh & JG_ISR_SHADOW_LEADS) ? (sh & 0xffu) : 0u;
  const uint32_t behind = (uint32_t)jg_lag_behind(R);  // (R >= 2 wherever a field is looked at: at most 21 bits)
  const bool run = jg_lag_base_is_run_hi(f);
  uint32_t isr = 1u << self, rare = 0;
#pragma unroll
  for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++) {
    if (r < R && r != self) {
      const uint32_t field = (uint32_t)jg_lag_field(w, r, R);
      const bool stays = (was >> r) & 1u;
      const uint32_t thr = stays ? leave32 : join32;
      if (!run && field < behind)
        isr |= (field <= thr ? 1u : 0u) << r;  // the common case: the lag IS the field
      else if (!run && field == behind && (stays ? leave : join) < (uint64_t)behind)
        ;  // too far BEHIND the head for its field, and the threshold is below the field limit: out, without a load
      else
        rare |= 1u << r;
    }
  }
  if (rare) {  // a BEHIND field under a wide threshold, an ABOVE field, a base that is run_hi: decoded exactly
    const uint64_t head = d.head[g], base = run ? d.run_hi[g] : head;
#pragma unroll
    for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++) {
      if ((rare >> r) & 1u) {
        const uint64_t lag = jg_isr_lag_exact(d, g, jg_lag_field(w, r, R), r, base, head);
        isr |= (lag <= (((was >> r) & 1u) ? leave : join) ? 1u : 0u) << r;
      }
    }
  }
  return isr | JG_ISR_SHADOW_LEADS;
}

// the largest lag over the members but the own slot of a leading slot whose head is `head` (0 at R = 1)
__device__ __forceinline__ uint64_t jg_isr_worst_lag(const JgDev& d, uint32_t g, uint32_t f, uint64_t w, uint64_t head) {
  const uint32_t R = d.R, self = (f & JGF_SELF_MASK) >> JGF_SELF_SHIFT;
  const bool run = jg_lag_base_is_run_hi(f);
  const uint64_t base = run ? d.run_hi[g] : head;
  uint64_t worst = 0;
#pragma unroll
  for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++) {
    if (r < R && r != self) {
      const uint64_t field = jg_lag_field(w, r, R);
      const uint64_t lag = (!run && !jg_lag_wide(field, R)) ? field : jg_isr_lag_exact(d, g, field, r, base, head);
      worst = lag > worst ? lag : worst;
    }
  }
  return worst;
}

struct JgIsrArgs {
  uint32_t g0, n;    // shard-local slots [g0, g0 + n)
  uint32_t add;      // added to every group written (a shard's first global slot)
  uint32_t peek;     // 1: the shadow is left alone
  uint64_t leave_lag, join_lag;
  uint32_t* shadow;  // [G]
  uint32_t* cnt;     // [tiles] the workgroup counts
  uint64_t* bsum;    // [tiles] the same, then (k_scan_block_sums) their exclusive prefixes
  jg_isr_row* out;   // [cap] (device)
  uint64_t cap;
  const uint32_t* gate;  // null, or a device word: nonzero = behave as under peek (a polled node step whose rows took the general path)
};

// a workgroup's rows: v[k] the view of slot t0 + k * JG_BLOCK as a shadow word, f[k] its flag word, w[k] its packed word,
// bit l of m[k] = the slot of lane l of this wave differs from its shadow.  (the loads first: three a row, twelve in
// flight per lane)
__device__ __forceinline__ void jg_isr_ballots(const JgDev& d, const JgIsrArgs& a, uint32_t* v, uint32_t* f, uint64_t* w, uint64_t* m) {
  const uint32_t t0 = blockIdx.x * JG_ISR_TILE + threadIdx.x;
  const uint32_t leave32 = jg_clamp32(a.leave_lag), join32 = jg_clamp32(a.join_lag);
  uint32_t sh[JG_ISR_ROWS];
#pragma unroll
  for (uint32_t k = 0; k < JG_ISR_ROWS; k++) {
    const uint32_t i = t0 + k * JG_BLOCK;
    const bool in = i < a.n;
    const uint32_t g = a.g0 + (in ? i : 0u);
    f[k] = in ? d.flags[g] : 0u;
    w[k] = in ? d.mlag[g] : 0ull;
    sh[k] = in ? a.shadow[g] : 0u;
  }
#pragma unroll
  for (uint32_t k = 0; k < JG_ISR_ROWS; k++) {
    const uint32_t i = t0 + k * JG_BLOCK;
    const bool in = i < a.n;
    v[k] = in ? jg_isr_word(d, a.leave_lag, a.join_lag, leave32, join32, a.g0 + i, f[k], w[k], sh[k]) : 0u;
    m[k] = __ballot(in && v[k] != sh[k]);
  }
}

__global__ __launch_bounds__(JG_BLOCK) void k_isr_count(JgDev d, JgIsrArgs a) {
  uint32_t v[JG_ISR_ROWS], f[JG_ISR_ROWS];
  uint64_t w[JG_ISR_ROWS], m[JG_ISR_ROWS];
  jg_isr_ballots(d, a, v, f, w, m);
  uint32_t c = 0;
#pragma unroll
  for (uint32_t k = 0; k < JG_ISR_ROWS; k++) c += __popcll(m[k]);
  const uint32_t t = jg_tile_count(c);
  if (threadIdx.x == 0) a.cnt[blockIdx.x] = t, a.bsum[blockIdx.x] = t;
}

// the write pass behind a feed's ballots (A: JgIsrArgs, or jg_isr_clock.h's JgIsrClockArgs): the rows of the slots of m
// below a.cap from `base` (the tile's prefix) on, and - unless peeking - their shadow words
template <class A>
__device__ __forceinline__ void jg_isr_write_rows(const JgDev& d, const A& a, uint64_t base, const uint32_t* v, const uint32_t* f, const uint64_t* w,
                                                  const uint64_t* m) {
  const uint32_t peek = jg_gated_peek(a.peek, a.gate);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t t0 = blockIdx.x * JG_ISR_TILE + threadIdx.x;
  uint64_t head[JG_ISR_ROWS];
#pragma unroll
  for (uint32_t k = 0; k < JG_ISR_ROWS; k++)  // the head of the slots that differ and lead: for their rows alone
    head[k] = (((m[k] >> lane) & 1ull) && v[k]) ? d.head[a.g0 + t0 + k * JG_BLOCK] : 0ull;
  const uint32_t R = d.R;
  uint64_t* out64 = (uint64_t*)a.out;
  jg_ranked_rows<JG_ISR_ROWS>(m, base, a.cap, [&](uint32_t k, uint64_t pos) {
    const uint32_t g = a.g0 + t0 + k * JG_BLOCK;
    const uint32_t self = (f[k] & JGF_SELF_MASK) >> JGF_SELF_SHIFT;
    uint32_t isr = 0, replicate = 0, state = 0;
    uint64_t worst = 0;
    if (v[k]) {
      isr = v[k] & 0xffu;
      const uint32_t in_sync = (uint32_t)__popcll((uint64_t)isr);
      replicate = (f[k] & JGF_REPL_MASK) >> JGF_REPL_SHIFT;
      state = JG_ISR_LEADS | (in_sync < R ? (uint32_t)JG_ISR_UNDER : 0u) | (in_sync < R / 2u + 1u ? (uint32_t)JG_ISR_BELOW_QUORUM : 0u);
      worst = jg_isr_worst_lag(d, g, f[k], w[k], head[k]);
    }
    // the row as three 8-byte pieces: {group, isr, replicate, state, self_slot} {head} {worst_lag}
    out64[pos * 3 + 0] = (uint64_t)(a.add + g) | (uint64_t)(isr | replicate << 8 | state << 16 | self << 24) << 32;
    out64[pos * 3 + 1] = head[k];
    out64[pos * 3 + 2] = worst;
    if (!peek) a.shadow[g] = v[k];
  });
}

__global__ __launch_bounds__(JG_BLOCK) void k_isr_write(JgDev d, JgIsrArgs a) {
  const uint64_t base = a.bsum[blockIdx.x];
  // (uniform over the workgroup) nothing differs here - the quiet engine's every workgroup - or it is all beyond cap
  if (a.cnt[blockIdx.x] == 0 || base >= a.cap) return;
  uint32_t v[JG_ISR_ROWS], f[JG_ISR_ROWS];
  uint64_t w[JG_ISR_ROWS], m[JG_ISR_ROWS];
  jg_isr_ballots(d, a, v, f, w, m);
  jg_isr_write_rows(d, a, base, v, f, w, m);
}

struct JgReplCensusArgs {
  uint32_t g0, n;  // shard-local slots [g0, g0 + n)
  uint32_t tiles;  // tiles of JG_REPL_CENSUS_TILE slots
  uint32_t parts;  // workgroups of k_repl_census = partial records (<= JG_REPL_CENSUS_PARTS)
  uint64_t lag_limit;
  uint64_t* part;  // [parts][JG_RC_WORDS]
  uint64_t* out;   // [JG_RC_WORDS]
};

__global__ __launch_bounds__(JG_BLOCK) void k_repl_census(JgDev d, JgReplCensusArgs a) {
  const uint32_t R = d.R;
  uint32_t c[JG_RC_MAX_LAG];  // the counted fields: wave-uniform (every lane adds the same popcount)
#pragma unroll
  for (uint32_t x = 0; x < JG_RC_MAX_LAG; x++) c[x] = 0;
  uint64_t max_lag[JG_MAX_REPLICAS], sum_lag[JG_MAX_REPLICAS], max_unc = 0;  // per lane
#pragma unroll
  for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++) max_lag[r] = 0, sum_lag[r] = 0;
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += a.parts) {  // (uniform over the workgroup)
    const uint32_t t0 = tile * JG_REPL_CENSUS_TILE + threadIdx.x;
    uint32_t f[JG_REPL_CENSUS_ROWS];
    uint64_t w[JG_REPL_CENSUS_ROWS];
#pragma unroll
    for (uint32_t k = 0; k < JG_REPL_CENSUS_ROWS; k++) {  // (the loads first)
      const uint32_t i = t0 + k * JG_BLOCK;
      const bool in = i < a.n;
      const uint32_t g = a.g0 + (in ? i : 0u);
      f[k] = in ? d.flags[g] : 0u;
      w[k] = in ? d.mlag[g] : 0ull;
    }
#pragma unroll
    for (uint32_t k = 0; k < JG_REPL_CENSUS_ROWS; k++) {
      const uint32_t i = t0 + k * JG_BLOCK;
      const uint32_t g = a.g0 + (i < a.n ? i : 0u);
      const bool led = i < a.n && jg_isr_leads(f[k]);
      const uint32_t self = (f[k] & JGF_SELF_MASK) >> JGF_SELF_SHIFT;
      uint64_t lag[JG_MAX_REPLICAS], unc = 0;
#pragma unroll
      for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++) lag[r] = 0;
      if (led) {
        const bool run = jg_lag_base_is_run_hi(f[k]);
        const uint64_t fc = jg_lag_field(w[k], R, R);
        bool rare = run || jg_lag_wide(fc, R);
#pragma unroll
        for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++) {
          if (r < R && r != self) {
            lag[r] = jg_lag_field(w[k], r, R);  // the common case: the lag IS the field
            rare = rare || jg_lag_wide(lag[r], R);
          }
        }
        unc = fc;  // ... and head - commit the commit's
        if (rare) {
          const uint64_t head = d.head[g], base = run ? d.run_hi[g] : head;
#pragma unroll
          for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++)
            if (r < R && r != self) lag[r] = jg_isr_lag_exact(d, g, lag[r], r, base, head);
          unc = head - jg_read_commit(d, g, f[k]);
        }
      }
      uint32_t in_sync = 1;
#pragma unroll
      for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++) {
        if (r < R) {  // (uniform)
          const bool member = led && r != self;
          const bool out = member && lag[r] > a.lag_limit;
          in_sync += member && !out ? 1u : 0u;
          c[JG_RC_OUT_OF_SYNC + r] += __popcll(__ballot(out));
          max_lag[r] = lag[r] > max_lag[r] ? lag[r] : max_lag[r];
          sum_lag[r] += lag[r];
        }
      }
      c[0] += __popcll(__ballot(led));
      c[1] += __popcll(__ballot(led && in_sync == R));
      c[2] += __popcll(__ballot(led && in_sync < R));
      c[3] += __popcll(__ballot(led && in_sync < R / 2u + 1u));
      max_unc = unc > max_unc ? unc : max_unc;
    }
  }
  uint64_t vals[JG_RC_WORDS];
#pragma unroll
  for (uint32_t x = 0; x < JG_RC_MAX_LAG; x++) vals[x] = c[x];
#pragma unroll
  for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++) {
    vals[JG_RC_MAX_LAG + r] = jg_wave_max64(max_lag[r]);
    vals[JG_RC_SUM_LAG + r] = jg_wave_sum64(sum_lag[r]);
  }
  vals[JG_RC_MAX_UNCOMMITTED] = jg_wave_max64(max_unc);
  jg_block_words<JG_RC_WORDS>(vals, [](uint32_t x) { return jg_rc_is_max(x); }, a.part);
}

__global__ __launch_bounds__(JG_BLOCK) void k_repl_census_sum(JgReplCensusArgs a) {
  jg_parts_reduce<JG_RC_WORDS>(a.part, a.parts, a.out, [](uint32_t x) { return jg_rc_is_max(x); });
}
