// jg_poll.h — gfx950 kernel of jg_engine_poll: the count passes of the three change feeds (jg_watch.h, jg_isr.h,
// jg_commits.h) as ONE pass over the slots.
//
// A tick of an event loop that consumes several feeds asks "what changed leader, whose in-sync set changed, what was
// committed or appended" of the same slots.  Asked separately the three count passes read 44 + 16 + 44 = 104 bytes per
// slot; here the flag word and mlag are read once: 88 bytes where all three are wanted.  The views, the shadows and the
// comparisons are the feeds' own functions - jg_lead_view / jg_lead_differs, jg_isr_word, jg_commit_view /
// jg_commit_differs / jg_commit_backlog_add - so the per-feed cnt[tile] / bsum[tile] this pass writes are exactly what
// k_watch_write, k_isr_write and k_commit_write index, and the commit backlog's partial records are what
// k_commit_backlog_sum adds up: those kernels run unchanged behind it.  The tails are jg_compact.h's.
//
//   k_poll_count<L, I, C>  the feeds wanted are launch-uniform template switches (two or three of them: a single feed has
//                          its own count kernel); commits_only and backlog are launch-uniform words of the commit feed's
//                          arguments, as in k_commit_count.  A workgroup strides over the tiles b, b + grid, ... and
//                          walks a tile of four rows as passes of JG_POLL_FLIGHT rows: every distinct column of the
//                          wanted feeds loaded once, all of a pass's loads in flight before the first use; per feed and
//                          row one __ballot and one __popcll per wave, both 32-bit halves of every compared word
//   k_poll_count_timed<L, C>  the same body (jg_poll_count_body<L, true, C, true>) with the replicas part under the TIME
//                          rule (jg_isr_clock.h; the part is implied, and wanted alone it is k_isrc_count's): the mask
//                          byte joins the loads of a pass, the word is jg_isrc_word as it stands - the stamp gathers and,
//                          unless peeking, the stores of the clocks behind its own conditions - and no lag policy is
//                          read: 89 bytes where all three are wanted and no clock runs.  Its cnt[tile] / bsum[tile] are
//                          what k_isrc_write indexes
//   k_scan_block_sums      (jg_sparse.h) one launch, one workgroup per wanted feed's bsum array
//   k_poll_header          (at the end of this file) a polled node step's answer but the rows as one block: one copy home
//
// THE GATE (ABI v21).  The passes that act on a feed's peek - the write passes and the two count passes that advance clocks -
// take an optional device word beside it (jg_gated_peek, jg_watch.h): null or zero, nothing changes; nonzero, the pass
// behaves as under JG_WATCH_PEEK.  A poll queued behind a node step whose rows took the general path is gated by that step's
// own general-row count: it writes no shadow and no clock, and is queued once more, ungated, behind the catch-up pass.
//
// Nothing here writes a column of the state machine or a shadow: the only stores are the scratch and, in the timed pass of
// a call that does not peek, the clocks - a slot is one lane's from load to store, no atomics.
#pragma once
#include "jg_commits.h"
#include "jg_isr.h"
#include "jg_isr_clock.h"
#include "jg_watch.h"

static_assert(JG_WATCH_TILE == JG_ISR_TILE && JG_ISR_TILE == JG_CMT_TILE, "the three write passes index one tiling");
#define JG_POLL_ROWS JG_CMT_ROWS
#define JG_POLL_TILE JG_CMT_TILE
static_assert(JG_ISR_TILE == JG_POLL_TILE, "k_isrc_write (jg_isr_clock.h) indexes the tiling of the timed pass");
// rows of a tile whose loads are in flight together: 22 dwords a row where all three feeds are wanted
#define JG_POLL_FLIGHT 4u
static_assert(JG_POLL_ROWS % JG_POLL_FLIGHT == 0, "a tile is whole passes");

struct JgPollArgs {
  uint32_t tiles;   // tiles of JG_POLL_TILE slots
  uint32_t parts;   // workgroups of k_poll_count (<= JG_CMT_PARTS)
  JgWatchArgs lw;   // the arguments of the wanted feeds' own write passes: g0 and n are the same in all of them
  JgIsrArgs ir;
  JgCommitArgs cm;
  JgIsrClockArgs ic;  // the replicas part under the time rule (k_poll_count_timed, k_isrc_write): in place of ir
};

// rows k0 .. k0 + JG_POLL_FLIGHT - 1 of a tile: c[x] += the slots of feed x (leaders, replicas, commits) that differ from
// its shadow, wave-uniform; bc / commits / appends: the commit backlog as k_commit_count keeps it.  T: the replicas part is
// under the time rule - leave32 is then caught_lag's 32-bit clamp, and with `advance` (the call does not peek and its gate
// is shut: uniform over the launch) the clocks of the rows advance
template <bool L, bool I, bool C, bool T>
__device__ __forceinline__ void jg_poll_rows(const JgDev& d, const JgPollArgs& a, uint32_t g0, uint32_t n, uint32_t tile, uint32_t k0,
                                             uint32_t leave32, uint32_t join32, uint32_t lane, bool advance, uint32_t* c, uint32_t* bc,
                                             uint64_t& commits, uint64_t& appends) {
  static_assert(I || !T, "the time rule is the replicas part's");
  const uint32_t t0 = tile * JG_POLL_TILE + k0 * JG_BLOCK + threadIdx.x;
  uint32_t f[JG_POLL_FLIGHT], ish[JG_POLL_FLIGHT], mk[JG_POLL_FLIGHT];
  uint64_t term[JG_POLL_FLIGHT], w[JG_POLL_FLIGHT], head[JG_POLL_FLIGHT], col[JG_POLL_FLIGHT];
  uint4 cold[JG_POLL_FLIGHT], lsh[JG_POLL_FLIGHT], csh[JG_POLL_FLIGHT];
#pragma unroll
  for (uint32_t k = 0; k < JG_POLL_FLIGHT; k++) {
    const uint32_t i = t0 + k * JG_BLOCK;
    const bool in = i < n;
    const uint32_t g = g0 + (in ? i : 0u);
    f[k] = in ? d.flags[g] : 0u;
    if (L) {
      term[k] = in ? d.term[g] : 0ull;
      cold[k] = in ? d.cold.v[g] : make_uint4(0, 0, 0, 0);
      lsh[k] = in ? a.lw.shadow[g] : make_uint4(0, 0, 0, 0);
    }
    if (I || C) w[k] = in ? d.mlag[g] : 0ull;
    if (I) ish[k] = in ? (T ? a.ic.shadow : a.ir.shadow)[g] : 0u;
    if (T) mk[k] = in ? (uint32_t)a.ic.mask[g] & ((1u << d.R) - 1u) : 0u;  // (no bit at or above R: no stamp column there)
    if (C) {
      head[k] = in ? d.head[g] : 0ull;
      col[k] = in ? d.commit[g] : 0ull;
      csh[k] = in ? a.cm.shadow[g] : make_uint4(0, 0, 0, 0);
    }
  }
  // (the loads stay up there: without an unconditional use the compiler sinks one behind a branch on the role)
#pragma unroll
  for (uint32_t k = 0; k < JG_POLL_FLIGHT; k++) {
    asm volatile("" ::"v"(f[k]));
    if (L) asm volatile("" ::"v"(term[k]), "v"(cold[k].y), "v"(lsh[k].x), "v"(lsh[k].z));
    if (I || C) asm volatile("" ::"v"(w[k]));
    if (I) asm volatile("" ::"v"(ish[k]));
    if (T) asm volatile("" ::"v"(mk[k]));
    if (C) asm volatile("" ::"v"(head[k]), "v"(col[k]), "v"(csh[k].x), "v"(csh[k].z));
  }
#pragma unroll
  for (uint32_t k = 0; k < JG_POLL_FLIGHT; k++) {
    const uint32_t i = t0 + k * JG_BLOCK;
    const bool in = i < n;
    if (L)  // jg_watch_ballots
      c[0] += __popcll(__ballot(in && jg_lead_differs(lsh[k], jg_lead_view(d, f[k], term[k], cold[k].y))));
    if (I && !T) {  // jg_isr_ballots
      const uint32_t v = in ? jg_isr_word(d, a.ir.leave_lag, a.ir.join_lag, leave32, join32, g0 + i, f[k], w[k], ish[k]) : 0u;
      c[1] += __popcll(__ballot(in && v != ish[k]));
    }
    if (T) {  // jg_isrc_ballots: a lane beyond n stores no clock either
      const uint32_t v = in ? jg_isrc_word(d, a.ic, leave32, join32, g0 + i, f[k], w[k], ish[k], mk[k], advance) : 0u;
      c[1] += __popcll(__ballot(in && v != ish[k]));
    }
    if (C) {  // jg_commit_ballots, and the backlog of k_commit_count
      const uint64_t cm = jg_commit_view(d, g0 + (in ? i : 0u), f[k], w[k], head[k], col[k]);
      const uint64_t m = __ballot(in && jg_commit_differs(csh[k], cm, head[k], a.cm.commits_only));
      c[2] += __popcll(m);
      if (a.cm.backlog) jg_commit_backlog_add((m >> lane) & 1ull, m, csh[k], cm, head[k], bc, commits, appends);  // (uniform over the launch)
    }
  }
}

// the count pass: T - the replicas part is under the time rule, its arguments a.ic in place of a.ir
template <bool L, bool I, bool C, bool T>
__device__ __forceinline__ void jg_poll_count_body(const JgDev& d, const JgPollArgs& a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g0 = T ? a.ic.g0 : L ? a.lw.g0 : a.ir.g0, n = T ? a.ic.n : L ? a.lw.n : a.ir.n;  // (two feeds at least: one of these is wanted)
  const uint32_t leave32 = jg_clamp32(T ? a.ic.caught_lag : a.ir.leave_lag), join32 = jg_clamp32(T ? a.ic.join_lag : a.ir.join_lag);
  const bool advance = T && !jg_gated_peek(a.ic.peek, a.ic.gate);  // (one scalar load per workgroup, outside the walk)
  uint32_t bc[4] = {0u, 0u, 0u, 0u};  // changed, committed, appended, rewound: wave-uniform
  uint64_t commits = 0, appends = 0;  // per lane
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += a.parts) {  // (uniform over the workgroup)
    uint32_t c[3] = {0u, 0u, 0u};
#pragma unroll
    for (uint32_t k0 = 0; k0 < JG_POLL_ROWS; k0 += JG_POLL_FLIGHT)
      jg_poll_rows<L, I, C, T>(d, a, g0, n, tile, k0, leave32, join32, lane, advance, c, bc, commits, appends);
    const uint32_t t = jg_tile_counts<3>(c);
    if (threadIdx.x < 3) {  // thread x: feed x's count of the tile (ONE guard: a branch per feed cost the pass 0.6 us at 1 M)
      const uint32_t x = threadIdx.x;
      if (L && x == 0) a.lw.cnt[tile] = t, a.lw.bsum[tile] = t;
      if (I && x == 1) (T ? a.ic.cnt : a.ir.cnt)[tile] = t, (T ? a.ic.bsum : a.ir.bsum)[tile] = t;
      if (C && x == 2) a.cm.cnt[tile] = t, a.cm.bsum[tile] = t;
    }
    __syncthreads();  // (jg_tile_counts' LDS is the next tile's too)
  }
  if (!C || !a.cm.backlog) return;
  const uint64_t vals[JG_CMT_WORDS] = {bc[0], bc[1], bc[2], bc[3], jg_wave_sum64(commits), jg_wave_sum64(appends)};
  jg_block_words<JG_CMT_WORDS>(vals, JgNeverMax(), a.cm.part);
}

template <bool L, bool I, bool C>
__global__ __launch_bounds__(JG_BLOCK) void k_poll_count(JgDev d, JgPollArgs a) {
  jg_poll_count_body<L, I, C, false>(d, a);
}

// k_poll_count's walk with the replicas part under the time rule: L / C the other feeds wanted (one of them at least)
template <bool L, bool C>
__global__ __launch_bounds__(JG_BLOCK) void k_poll_count_timed(JgDev d, JgPollArgs a) {
  static_assert(L || C, "a timed replicas part wanted alone is k_isrc_count's");
  jg_poll_count_body<L, true, C, true>(d, a);
}

// ---- the header of a poll that travels with a node step (jg_step_node_polled) -------------------------------------------
// Everything of the answer that is not a row, as ONE block of 8-byte words per kept-step set: one copy brings it home.
#define JG_PH_TOTAL 0u                                  // [3] the slots of each feed that differ (leaders, replicas, commits)
#define JG_PH_GIVEN 3u                                  // [3] min(cap, total): the rows delivered
#define JG_PH_BACKLOG 6u                                // [JG_CMT_WORDS]
#define JG_PH_CENSUS (JG_PH_BACKLOG + JG_CMT_WORDS)     // [JG_CENSUS_WORDS]
#define JG_PH_REPL (JG_PH_CENSUS + JG_CENSUS_WORDS)     // [JG_RC_WORDS]
#define JG_PH_GATE (JG_PH_REPL + JG_RC_WORDS)           // the gate's verdict: the step's general-path rows as this pass saw them
#define JG_PH_WORDS (JG_PH_GATE + 1u)
static_assert(JG_PH_WORDS <= JG_BLOCK, "one thread a word");

struct JgPollHeaderArgs {
  const uint64_t* total;    // what k_scan_block_sums left: one word per job
  uint32_t job[3];          // feed x's job, or 0xffffffff: not wanted
  uint32_t pad;
  uint64_t cap[3];
  const uint64_t* backlog;  // [JG_CMT_WORDS] or null
  const uint64_t* census;   // [JG_CENSUS_WORDS] or null
  const uint64_t* repl;     // [JG_RC_WORDS] or null
  const uint32_t* gate;     // or null
  uint64_t* out;            // [JG_PH_WORDS]
};

// one workgroup, one thread a word; a part that is not wanted is zeros
__global__ __launch_bounds__(JG_BLOCK) void k_poll_header(JgPollHeaderArgs a) {
  const uint32_t x = threadIdx.x;
  if (x >= JG_PH_WORDS) return;
  uint64_t v = 0;
  if (x < JG_PH_BACKLOG) {
    const uint32_t feed = x < JG_PH_GIVEN ? x : x - JG_PH_GIVEN;
    const uint64_t t = a.job[feed] != 0xffffffffu ? a.total[a.job[feed]] : 0ull;
    v = x < JG_PH_GIVEN ? t : (t < a.cap[feed] ? t : a.cap[feed]);
  } else if (x < JG_PH_CENSUS) {
    v = a.backlog ? a.backlog[x - JG_PH_BACKLOG] : 0ull;
  } else if (x < JG_PH_REPL) {
    v = a.census ? a.census[x - JG_PH_CENSUS] : 0ull;
  } else if (x < JG_PH_GATE) {
    v = a.repl ? a.repl[x - JG_PH_REPL] : 0ull;
  } else {
    v = a.gate ? *a.gate : 0u;
  }
  a.out[x] = v;
}
