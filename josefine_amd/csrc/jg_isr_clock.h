// jg_isr_clock.h — gfx950 kernels of jg_engine_watch_replicas_timed: the replication feed (jg_isr.h) under the TIME rule -
// a member leaves the in-sync set of a partition this engine leads once it has been behind for longer than max_behind_ms
// (replica.lag.time.max.ms), not once it is some number of blocks behind.
//
// The rows, the SHADOW word {isr | LEADS << 8} and the compaction are jg_isr.h's: the two calls are one feed.  What is new
// is the CLOCKS, feed memory of their own allocated zero-filled at the first timed call:
//   stamp[r][g]  8 bytes per member and slot ([R][G] like match_wide): 0 = "not behind at the last sample", else now_ms + 1
//                of the first sample that saw the member with lag > caught_lag
//   mask[g]      1 byte per slot: bit r = stamp[r][g] != 0.  It is what keeps the steady state off the stamp columns
// Per sample, slot g that leads and member r but the own slot:
//   c' = lag_r <= caught_lag ? 0 : (stamp ? stamp : now_ms + 1);   behind_ms = c' && now_ms + 1 > c' ? now_ms + 1 - c' : 0
//   in_r = was_r ? behind_ms <= max_behind_ms : lag_r <= join_lag      (was_r: the shadow says the slot led and had bit r)
// and of a slot that does not lead every clock becomes 0.  Both lag predicates are jg_isr_word's, asked with an empty
// shadow (every member "joins") and the one threshold: the escapes and a base that is run_hi are decoded there, exactly.
// A stamp is LOADED only for a member the shadow holds that is behind now and whose mask bit is set - any other clock
// is 0, or starts now, or does not matter; a stamp is STORED only where it changes (behind & ~mask: started, mask &
// ~behind: cleared), the mask byte only where it changes.  With every follower caught up and no clock running a slot
// costs the flag word, mlag, the shadow word and the mask byte: 17 bytes, against the lag feed's 16.
//
//   k_isrc_count       pass 1 of the compaction over "view != shadow", and - unless peeking - THE pass that advances the
//                      clocks, of every slot of the range: time passes for a row that is not delivered.  Advancing twice at
//                      one now_ms on unchanged state stores nothing the second time
//   k_scan_block_sums  (jg_sparse.h) the workgroup counts -> exclusive prefixes and the total
//   k_isrc_write       pass 2: a workgroup with nothing to report or wholly beyond `cap` returns after two loads; else the
//                      same view re-derived from the clocks already advanced (peeking: from the would-be clocks - the
//                      same function of memory nobody wrote), then jg_isr_write_rows (jg_isr.h): the rows as k_isr_write
//                      writes them, and - unless peeking - the shadow word of exactly the delivered slots.  It stores no
//                      clock
//
// A slot is one lane's from load to store in both passes; no atomics, no scratch.  Nothing here writes a column of the
// state machine: the only stores are the scratch, the rows, the shadow and the clocks.
#pragma once
#include "jg_isr.h"

struct JgIsrClockArgs {
  uint32_t g0, n;      // shard-local slots [g0, g0 + n)
  uint32_t add;        // added to every group written (a shard's first global slot)
  uint32_t peek;       // 1: clocks and shadow are left alone
  uint64_t now1;       // now_ms + 1 (now_ms < UINT64_MAX)
  uint64_t max_behind_ms, caught_lag, join_lag;
  uint32_t* shadow;    // [G]
  uint64_t* stamp;     // [R][G]
  uint8_t* mask;       // [G]
  uint32_t* cnt;       // [tiles] the workgroup counts
  uint64_t* bsum;      // [tiles] the same, then (k_scan_block_sums) their exclusive prefixes
  jg_isr_row* out;     // [cap] (device)
  uint64_t cap;
  const uint32_t* gate;  // null, or a device word: nonzero = behave as under peek (a polled node step whose rows took the general path)
};

// The in-sync set of slot g under the time rule as the shadow holds it (isr | LEADS, 0 for a slot that does not lead) from
// its flag word f, its packed word w, its shadow word sh and its mask byte mk.  `advance`: store the clocks of this sample
// (the count pass of a call that does not peek); the view is the same either way.
__device__ __forceinline__ uint32_t jg_isrc_word(const JgDev& d, const JgIsrClockArgs& a, uint32_t caught32, uint32_t join32, uint32_t g, uint32_t f,
                                                 uint64_t w, uint32_t sh, uint32_t mk, bool advance) {
  // bit r = lag_r <= caught_lag (the own slot's set, LEADS above them); 0: the slot does not lead
  const uint32_t cw = jg_isr_word(d, a.caught_lag, a.caught_lag, caught32, caught32, g, f, w, 0u);
  const size_t G = d.G;
  if (!cw) {  // every clock of the slot becomes 0
    if (advance && mk) {
#pragma unroll
      for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++)
        if ((mk >> r) & 1u) a.stamp[(size_t)r * G + g] = 0ull;
      a.mask[g] = 0;
    }
    return 0u;
  }
  const uint32_t R = d.R, self = (f & JGF_SELF_MASK) >> JGF_SELF_SHIFT;
  const uint32_t members = ((1u << R) - 1u) & ~(1u << self);
  const uint32_t behind = members & ~cw;  // lag_r > caught_lag
  // bit r = lag_r <= join_lag
  const uint32_t jw = a.join_lag == a.caught_lag ? cw : jg_isr_word(d, a.join_lag, a.join_lag, join32, join32, g, f, w, 0u);
  const uint32_t was = (sh & JG_ISR_SHADOW_LEADS) ? (sh & 0xffu) : 0u;
  // a member's time behind is not 0 only where its clock ran before this sample: the one case that reads a stamp
  uint32_t timed = was & behind & mk, expired = 0;
#pragma unroll
  for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++) {
    if ((timed >> r) & 1u) {
      const uint64_t c = a.stamp[(size_t)r * G + g];
      const uint64_t behind_ms = a.now1 > c ? a.now1 - c : 0ull;  // (saturating: a clock that steps back evicts nobody)
      expired |= (behind_ms > a.max_behind_ms ? 1u : 0u) << r;
    }
  }
  if (advance) {
    const uint32_t keep = mk & ~members;  // (the own slot's clock is ignored: neither read nor written)
    const uint32_t start = behind & ~mk, clear = mk & members & ~behind;
    if (start | clear) {
#pragma unroll
      for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++) {
        if ((start >> r) & 1u) a.stamp[(size_t)r * G + g] = a.now1;
        if ((clear >> r) & 1u) a.stamp[(size_t)r * G + g] = 0ull;
      }
      a.mask[g] = (uint8_t)(keep | behind);
    }
  }
  const uint32_t isr = (1u << self) | (members & ((was & ~expired) | (~was & jw)));
  return isr | JG_ISR_SHADOW_LEADS;
}

// a workgroup's rows as jg_isr_ballots states them: v[k] the view of slot t0 + k * JG_BLOCK as a shadow word, f[k] its flag
// word, w[k] its packed word, bit l of m[k] = the slot of lane l of this wave differs from its shadow.  (the loads first:
// four a row; a lane beyond n loads nothing)
__device__ __forceinline__ void jg_isrc_ballots(const JgDev& d, const JgIsrClockArgs& a, bool advance, uint32_t* v, uint32_t* f, uint64_t* w, uint64_t* m) {
  const uint32_t t0 = blockIdx.x * JG_ISR_TILE + threadIdx.x;
  const uint32_t caught32 = jg_clamp32(a.caught_lag), join32 = jg_clamp32(a.join_lag);
  const uint32_t members_all = (1u << d.R) - 1u;  // (a mask byte never holds a bit at or above R: no stamp column there)
  uint32_t sh[JG_ISR_ROWS], mk[JG_ISR_ROWS];
#pragma unroll
  for (uint32_t k = 0; k < JG_ISR_ROWS; k++) {
    const uint32_t i = t0 + k * JG_BLOCK;
    const bool in = i < a.n;
    const uint32_t g = a.g0 + (in ? i : 0u);
    f[k] = in ? d.flags[g] : 0u;
    w[k] = in ? d.mlag[g] : 0ull;
    sh[k] = in ? a.shadow[g] : 0u;
    mk[k] = in ? (uint32_t)a.mask[g] & members_all : 0u;
  }
#pragma unroll
  for (uint32_t k = 0; k < JG_ISR_ROWS; k++) {
    const uint32_t i = t0 + k * JG_BLOCK;
    const bool in = i < a.n;
    v[k] = in ? jg_isrc_word(d, a, caught32, join32, a.g0 + i, f[k], w[k], sh[k], mk[k], advance) : 0u;
    m[k] = __ballot(in && v[k] != sh[k]);
  }
}

__global__ __launch_bounds__(JG_BLOCK) void k_isrc_count(JgDev d, JgIsrClockArgs a) {
  uint32_t v[JG_ISR_ROWS], f[JG_ISR_ROWS];
  uint64_t w[JG_ISR_ROWS], m[JG_ISR_ROWS];
  jg_isrc_ballots(d, a, !jg_gated_peek(a.peek, a.gate), v, f, w, m);
  uint32_t c = 0;
#pragma unroll
  for (uint32_t k = 0; k < JG_ISR_ROWS; k++) c += __popcll(m[k]);
  const uint32_t t = jg_tile_count(c);
  if (threadIdx.x == 0) a.cnt[blockIdx.x] = t, a.bsum[blockIdx.x] = t;
}

__global__ __launch_bounds__(JG_BLOCK) void k_isrc_write(JgDev d, JgIsrClockArgs a) {
  const uint64_t base = a.bsum[blockIdx.x];
  // (uniform over the workgroup) nothing differs here - the quiet engine's every workgroup - or it is all beyond cap
  if (a.cnt[blockIdx.x] == 0 || base >= a.cap) return;
  uint32_t v[JG_ISR_ROWS], f[JG_ISR_ROWS];
  uint64_t w[JG_ISR_ROWS], m[JG_ISR_ROWS];
  jg_isrc_ballots(d, a, false, v, f, w, m);
  jg_isr_write_rows(d, a, base, v, f, w, m);
}
