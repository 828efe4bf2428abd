// jg_commits.h — gfx950 kernels of jg_engine_watch_commits: which partitions' commit index (the high watermark) or head
// moved since the feed last delivered them, and from where to where - the fsm_tx the dense entry points do not queue.
//
// The COMMIT VIEW of a slot is (commit, head) exactly as jg_read_state returns JG_FIELD_COMMIT / JG_FIELD_HEAD: the head
// column, and the commit column - of a leader the commit field of the packed word d.mlag (jg_device.h), a lag below the
// head in the common case, decoded exactly under a branch where the field is an escape or the base is run_hi.  The SHADOW
// is 16 bytes per slot {commit_from, head_from} as last delivered, allocated at the engine's first watch; zero-filled it
// says "genesis only".
//
//   k_commit_count        stream compaction over "view != shadow" (the skeleton of both passes: jg_compact.h), pass 1: per
//                         tile of 1024 slots the number that differ (a 64-bit __ballot and a __popcll per wave and row of
//                         256 slots); 44 bytes read per slot - the flag word, head, mlag, the commit column and the
//                         shadow, all of a lane's four rows in flight before the first use.  A workgroup takes the tiles
//                         b, b + grid, ..., so where the backlog is wanted (launch-uniform) there are at most JG_CMT_PARTS
//                         partial records (jg_block_words): four counts by ballots, two sums by jg_wave_sum64
//   k_scan_block_sums     (jg_sparse.h) the tile counts -> exclusive prefixes and the total
//   k_commit_write        pass 2: a workgroup with nothing to report or wholly beyond `cap` returns after two loads; else
//                         the same ballots, the term of the slots that differ, the first `cap` rows ascending
//                         (jg_ranked_rows) as three 16-byte stores, and - unless peeking - the shadow of exactly those slots
//   k_commit_backlog_sum  the partial records -> the backlog (jg_parts_reduce: one workgroup; no atomics anywhere)
// The per-slot pieces - jg_commit_view, jg_commit_differs, jg_commit_backlog_add - are the fused pass's too (jg_poll.h).
//
// Nothing here writes a column of the state machine: the only stores are the scratch, the rows and the shadow.
#pragma once
#include "jg_device.h"
#include "jg_lookup.h"  // jg_u32x4
#include "jg_read.h"    // jg_read_commit
#include "jg_sparse.h"  // JgScanJob, k_scan_block_sums
#include "jg_watch.h"   // jg_gated_peek (and jg_compact.h)

#define JG_CMT_ROWS 4u  // rows of JG_BLOCK slots per tile of the watch passes (44 bytes in flight per lane and row)
#define JG_CMT_TILE (JG_BLOCK * JG_CMT_ROWS)
// the most workgroups - partial records of the backlog - of the count pass: four a CU on 256 CUs (JG_REPL_CENSUS_PARTS)
#define JG_CMT_PARTS 1024u
#define JG_CMT_WORDS 6u  // jg_commit_backlog as the words the kernels add up, in order
static_assert(sizeof(jg_commit_backlog) == JG_CMT_WORDS * 8, "jg_commit_backlog is the backlog words in order");
static_assert(sizeof(jg_commit_row) == 48, "jg_commit_row is three 16-byte pieces");

struct JgCommitArgs {
  uint32_t g0, n;         // shard-local slots [g0, g0 + n)
  uint32_t add;           // added to every group written (a shard's first global slot)
  uint32_t peek;          // 1: the shadow is left alone
  uint32_t commits_only;  // 1: a slot differs iff its commit does
  uint32_t backlog;       // 1: the count pass writes its partial records
  uint32_t tiles;         // tiles of JG_CMT_TILE slots
  uint32_t parts;         // workgroups of k_commit_count (<= JG_CMT_PARTS)
  uint4* shadow;          // [G] {commit_from, head_from}
  uint32_t* cnt;          // [tiles] the tile counts
  uint64_t* bsum;         // [tiles] the same, then (k_scan_block_sums) their exclusive prefixes
  uint64_t* part;         // [parts][JG_CMT_WORDS]
  uint64_t* sum;          // [JG_CMT_WORDS] the backlog
  uint4* out;             // [cap] rows of three 16-byte pieces (device)
  uint64_t cap;
  const uint32_t* gate;  // null, or a device word: nonzero = behave as under peek (a polled node step whose rows took the general path)
};

__device__ __forceinline__ uint64_t jg_cmt_u64(uint32_t lo, uint32_t hi) { return (uint64_t)lo | (uint64_t)hi << 32; }

// the commit of slot g (in range) from its flag word f, its packed word w, its head and its commit column
__device__ __forceinline__ uint64_t jg_commit_view(const JgDev& d, uint32_t g, uint32_t f, uint64_t w, uint64_t head, uint64_t col) {
  const uint32_t R = d.R;
  const bool leader = (f & JGF_ROLE_MASK) == JG_ROLE_LEADER;
  const uint64_t fc = jg_lag_field(w, R, R);
  uint64_t c = leader ? head - fc : col;  // the common case: a leader's commit IS head - field
  if (leader && (jg_lag_wide(fc, R) || jg_lag_base_is_run_hi(f))) c = jg_read_commit(d, g, f);  // rare: exact
  return c;
}
__device__ __forceinline__ bool jg_commit_differs(const uint4& sh, uint64_t commit, uint64_t head, uint32_t commits_only) {
  return sh.x != (uint32_t)commit || sh.y != (uint32_t)(commit >> 32) ||
         (!commits_only && (sh.z != (uint32_t)head || sh.w != (uint32_t)(head >> 32)));
}
// the backlog of one row of 64 slots: bc = changed, committed, appended, rewound, wave-uniform (every lane adds the same
// popcount); commits / appends per lane.  on: this lane's bit of the row's ballot m
__device__ __forceinline__ void jg_commit_backlog_add(bool on, uint64_t m, const uint4& sh, uint64_t commit, uint64_t head, uint32_t* bc,
                                                      uint64_t& commits, uint64_t& appends) {
  const uint64_t cf = jg_cmt_u64(sh.x, sh.y), hf = jg_cmt_u64(sh.z, sh.w);
  const bool up_c = on && commit > cf, up_h = on && head > hf;
  bc[0] += __popcll(m);
  bc[1] += __popcll(__ballot(up_c));
  bc[2] += __popcll(__ballot(up_h));
  bc[3] += __popcll(__ballot(on && (commit < cf || head < hf)));
  commits += up_c ? commit - cf : 0ull;
  appends += up_h ? head - hf : 0ull;
}

// a tile's rows: of slot t0 + k * JG_BLOCK the flag word f[k], the view commit[k] / head[k], the shadow sh[k]; bit l of
// m[k] = the slot of lane l of this wave differs from its shadow.  (the loads first: five a row, twenty in flight per
// lane - mlag AND the commit column whatever the role: a second, dependent trip costs more than 8 bytes per slot)
__device__ __forceinline__ void jg_commit_ballots(const JgDev& d, const JgCommitArgs& a, uint32_t tile, uint32_t* f, uint64_t* commit,
                                                  uint64_t* head, uint4* sh, uint64_t* m) {
  const uint32_t t0 = tile * JG_CMT_TILE + threadIdx.x;
  uint64_t w[JG_CMT_ROWS], col[JG_CMT_ROWS];
#pragma unroll
  for (uint32_t k = 0; k < JG_CMT_ROWS; k++) {
    const uint32_t i = t0 + k * JG_BLOCK;
    const bool in = i < a.n;
    const uint32_t g = a.g0 + (in ? i : 0u);
    f[k] = in ? d.flags[g] : 0u;
    head[k] = in ? d.head[g] : 0ull;
    w[k] = in ? d.mlag[g] : 0ull;
    col[k] = in ? d.commit[g] : 0ull;
    sh[k] = in ? a.shadow[g] : make_uint4(0, 0, 0, 0);
  }
  // (the loads stay up there: without an unconditional use the compiler sinks one behind the branch on the role)
#pragma unroll
  for (uint32_t k = 0; k < JG_CMT_ROWS; k++) asm volatile("" ::"v"(f[k]), "v"(head[k]), "v"(w[k]), "v"(col[k]), "v"(sh[k].x), "v"(sh[k].z));
#pragma unroll
  for (uint32_t k = 0; k < JG_CMT_ROWS; k++) {
    const uint32_t i = t0 + k * JG_BLOCK;
    const bool in = i < a.n;
    commit[k] = jg_commit_view(d, a.g0 + (in ? i : 0u), f[k], w[k], head[k], col[k]);
    m[k] = __ballot(in && jg_commit_differs(sh[k], commit[k], head[k], a.commits_only));
  }
}

__global__ __launch_bounds__(JG_BLOCK) void k_commit_count(JgDev d, JgCommitArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t bc[4] = {0u, 0u, 0u, 0u};  // changed, committed, appended, rewound: wave-uniform
  uint64_t commits = 0, appends = 0;  // per lane
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += a.parts) {  // (uniform over the workgroup)
    uint32_t f[JG_CMT_ROWS];
    uint64_t commit[JG_CMT_ROWS], head[JG_CMT_ROWS], m[JG_CMT_ROWS];
    uint4 sh[JG_CMT_ROWS];
    jg_commit_ballots(d, a, tile, f, commit, head, sh, m);
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < JG_CMT_ROWS; k++) c += __popcll(m[k]);
    if (a.backlog) {  // (uniform over the launch)
#pragma unroll
      for (uint32_t k = 0; k < JG_CMT_ROWS; k++)
        jg_commit_backlog_add((m[k] >> lane) & 1ull, m[k], sh[k], commit[k], head[k], bc, commits, appends);
    }
    const uint32_t t = jg_tile_count(c);
    if (threadIdx.x == 0) a.cnt[tile] = t, a.bsum[tile] = t;
    __syncthreads();  // (jg_tile_count's LDS is the next tile's too)
  }
  if (!a.backlog) return;
  const uint64_t vals[JG_CMT_WORDS] = {bc[0], bc[1], bc[2], bc[3], jg_wave_sum64(commits), jg_wave_sum64(appends)};
  jg_block_words<JG_CMT_WORDS>(vals, JgNeverMax(), a.part);
}

__global__ __launch_bounds__(JG_BLOCK) void k_commit_write(JgDev d, JgCommitArgs a) {
  const uint64_t base = a.bsum[blockIdx.x];
  // (uniform over the workgroup) nothing differs here - the quiet engine's every workgroup - or it is all beyond cap
  if (a.cnt[blockIdx.x] == 0 || base >= a.cap) return;
  uint32_t f[JG_CMT_ROWS];
  uint64_t commit[JG_CMT_ROWS], head[JG_CMT_ROWS], m[JG_CMT_ROWS];
  uint4 sh[JG_CMT_ROWS];
  jg_commit_ballots(d, a, blockIdx.x, f, commit, head, sh, m);
  const uint32_t peek = jg_gated_peek(a.peek, a.gate);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t t0 = blockIdx.x * JG_CMT_TILE + threadIdx.x;
  uint64_t term[JG_CMT_ROWS];
#pragma unroll
  for (uint32_t k = 0; k < JG_CMT_ROWS; k++)  // the term of the slots that differ: for their rows alone
    term[k] = ((m[k] >> lane) & 1ull) ? d.term[a.g0 + t0 + k * JG_BLOCK] : 0ull;
  jg_u32x4* out = (jg_u32x4*)a.out;
  auto lo = [](uint64_t x) { return (uint32_t)x; };
  auto hi = [](uint64_t x) { return (uint32_t)(x >> 32); };
  jg_ranked_rows<JG_CMT_ROWS>(m, base, a.cap, [&](uint32_t k, uint64_t pos) {
    const uint32_t g = a.g0 + t0 + k * JG_BLOCK;
    const uint32_t role = f[k] & JGF_ROLE_MASK, fault = (f[k] & JGF_FAULT_MASK) >> JGF_FAULT_SHIFT, self = (f[k] & JGF_SELF_MASK) >> JGF_SELF_SHIFT;
    const uint64_t cf = jg_cmt_u64(sh[k].x, sh[k].y), hf = jg_cmt_u64(sh[k].z, sh[k].w);
    const uint32_t state = (commit[k] > cf ? (uint32_t)JG_CMT_COMMITTED : 0u) | (head[k] > hf ? (uint32_t)JG_CMT_APPENDED : 0u) |
                           (commit[k] < cf || head[k] < hf ? (uint32_t)JG_CMT_REWOUND : 0u) |
                           (role == JG_ROLE_LEADER && fault == 0 ? (uint32_t)JG_CMT_LEADS : 0u) |
                           (fault == JG_FAULT_VACANT ? (uint32_t)JG_CMT_VACANT : fault ? (uint32_t)JG_CMT_FAULTED : 0u);
    // the row as three 16-byte pieces: {group, role | state | fault | self_slot, term} {commit_from, commit} {head_from, head}
    out[pos * 3 + 0] = jg_u32x4{a.add + g, role | state << 8 | fault << 16 | self << 24, lo(term[k]), hi(term[k])};
    out[pos * 3 + 1] = jg_u32x4{sh[k].x, sh[k].y, lo(commit[k]), hi(commit[k])};
    out[pos * 3 + 2] = jg_u32x4{sh[k].z, sh[k].w, lo(head[k]), hi(head[k])};
    if (!peek) a.shadow[g] = make_uint4(lo(commit[k]), hi(commit[k]), lo(head[k]), hi(head[k]));
  });
}

__global__ __launch_bounds__(JG_BLOCK) void k_commit_backlog_sum(JgCommitArgs a) {
  jg_parts_reduce<JG_CMT_WORDS>(a.part, a.parts, a.sum, JgNeverMax());
}
