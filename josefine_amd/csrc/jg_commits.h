// jg_commits.h — gfx950 kernels of jg_engine_watch_commits: which partitions' commit index (the high watermark) or head
// moved since the feed last delivered them, and from where to where - the fsm_tx the dense entry points do not queue.
//
// The COMMIT VIEW of a slot is (commit, head) exactly as jg_read_state returns JG_FIELD_COMMIT / JG_FIELD_HEAD: the head
// column, and the commit column - of a leader the commit field of the packed word d.mlag (jg_device.h), a lag below the
// head in the common case, decoded exactly under a branch where the field is an escape or the base is run_hi.  The SHADOW
// is 16 bytes per slot {commit_from, head_from} as last delivered, allocated at the engine's first watch; zero-filled it
// says "genesis only".
//
//   k_commit_count        stream compaction over "view != shadow", pass 1: per tile of 1024 slots the number that differ
//                         (a 64-bit __ballot and a __popcll per wave and row of 256 slots); 44 bytes read per slot - the
//                         flag word, head, mlag, the commit column and the shadow, all of a lane's four rows in flight
//                         before the first use.  A workgroup takes the tiles b, b + grid, ..., so where the backlog is
//                         wanted (launch-uniform) there are at most JG_CMT_PARTS partial records: four counts by ballots,
//                         two sums by jg_wave_sum64
//   k_scan_block_sums     (jg_sparse.h) the tile counts -> exclusive prefixes and the total
//   k_commit_write        pass 2: a workgroup with nothing to report or wholly beyond `cap` returns after two loads; else
//                         the same ballots, the term of the slots that differ, the ranks within a wave from the ballot, the
//                         wave offsets through LDS; the first `cap` rows ascending as three 16-byte stores, and - unless
//                         peeking - the shadow of exactly those slots
//   k_commit_backlog_sum  the partial records -> the backlog (one workgroup; no atomics anywhere)
//
// Nothing here writes a column of the state machine: the only stores are the scratch, the rows and the shadow.
#pragma once
#include "jg_device.h"
#include "jg_lookup.h"  // jg_u32x4
#include "jg_read.h"    // jg_read_commit
#include "jg_sparse.h"  // JgScanJob, k_scan_block_sums
#include "jg_watch.h"   // jg_wave_sum64

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

// a tile's rows: of slot t0 + k * JG_BLOCK the flag word f[k], the view commit[k] / head[k], the shadow sh[k]; bit l of
// m[k] = the slot of lane l of this wave differs from its shadow.  (the loads first: five a row, twenty in flight per
// lane - mlag AND the commit column whatever the role: a second, dependent trip costs more than 8 bytes per slot)
__device__ __forceinline__ void jg_commit_ballots(const JgDev& d, const JgCommitArgs& a, uint32_t tile, uint32_t* f, uint64_t* commit,
                                                  uint64_t* head, uint4* sh, uint64_t* m) {
  const uint32_t t0 = tile * JG_CMT_TILE + threadIdx.x;
  const uint32_t R = d.R;
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
    const bool leader = (f[k] & JGF_ROLE_MASK) == JG_ROLE_LEADER;
    const uint64_t fc = jg_lag_field(w[k], R, R);
    uint64_t c = leader ? head[k] - fc : col[k];  // the common case: a leader's commit IS head - field
    if (leader && (jg_lag_wide(fc, R) || jg_lag_base_is_run_hi(f[k]))) c = jg_read_commit(d, a.g0 + (in ? i : 0u), f[k]);  // rare: exact
    commit[k] = c;
    const bool differs = sh[k].x != (uint32_t)c || sh[k].y != (uint32_t)(c >> 32) ||
                         (!a.commits_only && (sh[k].z != (uint32_t)head[k] || sh[k].w != (uint32_t)(head[k] >> 32)));
    m[k] = __ballot(in && differs);
  }
}

__global__ __launch_bounds__(JG_BLOCK) void k_commit_count(JgDev d, JgCommitArgs a) {
  __shared__ uint32_t wave_n[JG_BLOCK / 64];
  __shared__ uint64_t wave_b[JG_BLOCK / 64][JG_CMT_WORDS];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t bc[4] = {0u, 0u, 0u, 0u};  // changed, committed, appended, rewound: wave-uniform (every lane adds the same popcount)
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
      for (uint32_t k = 0; k < JG_CMT_ROWS; k++) {
        const bool on = (m[k] >> lane) & 1ull;
        const uint64_t cf = jg_cmt_u64(sh[k].x, sh[k].y), hf = jg_cmt_u64(sh[k].z, sh[k].w);
        const bool up_c = on && commit[k] > cf, up_h = on && head[k] > hf;
        bc[0] += __popcll(m[k]);
        bc[1] += __popcll(__ballot(up_c));
        bc[2] += __popcll(__ballot(up_h));
        bc[3] += __popcll(__ballot(on && (commit[k] < cf || head[k] < hf)));
        commits += up_c ? commit[k] - cf : 0ull;
        appends += up_h ? head[k] - hf : 0ull;
      }
    }
    if (lane == 0) wave_n[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t t = 0;
#pragma unroll
      for (uint32_t x = 0; x < JG_BLOCK / 64; x++) t += wave_n[x];
      a.cnt[tile] = t;
      a.bsum[tile] = t;
    }
    __syncthreads();  // (wave_n is the next tile's too)
  }
  if (!a.backlog) return;
  commits = jg_wave_sum64(commits);
  appends = jg_wave_sum64(appends);
  if (lane == 0) {
#pragma unroll
    for (uint32_t x = 0; x < 4; x++) wave_b[wave][x] = bc[x];
    wave_b[wave][4] = commits;
    wave_b[wave][5] = appends;
  }
  __syncthreads();
  if (threadIdx.x < JG_CMT_WORDS) {
    uint64_t t = 0;
#pragma unroll
    for (uint32_t x = 0; x < JG_BLOCK / 64; x++) t += wave_b[x][threadIdx.x];
    a.part[(size_t)blockIdx.x * JG_CMT_WORDS + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(JG_BLOCK) void k_commit_write(JgDev d, JgCommitArgs a) {
  __shared__ uint32_t wave_n[JG_CMT_ROWS][JG_BLOCK / 64];
  uint64_t base = a.bsum[blockIdx.x];
  // (uniform over the workgroup) nothing differs here - the quiet engine's every workgroup - or it is all beyond cap
  if (a.cnt[blockIdx.x] == 0 || base >= a.cap) return;
  uint32_t f[JG_CMT_ROWS];
  uint64_t commit[JG_CMT_ROWS], head[JG_CMT_ROWS], m[JG_CMT_ROWS];
  uint4 sh[JG_CMT_ROWS];
  jg_commit_ballots(d, a, blockIdx.x, f, commit, head, sh, m);
  const uint32_t peek = jg_gated_peek(a.peek, a.gate);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t t0 = blockIdx.x * JG_CMT_TILE + threadIdx.x;
  uint64_t term[JG_CMT_ROWS];
#pragma unroll
  for (uint32_t k = 0; k < JG_CMT_ROWS; k++)  // the term of the slots that differ: for their rows alone
    term[k] = ((m[k] >> lane) & 1ull) ? d.term[a.g0 + t0 + k * JG_BLOCK] : 0ull;
  if (lane == 0) {
#pragma unroll
    for (uint32_t k = 0; k < JG_CMT_ROWS; k++) wave_n[k][wave] = __popcll(m[k]);
  }
  __syncthreads();
  const uint64_t below = lane ? (~0ull >> (64u - lane)) : 0ull;  // the lanes below this one
  jg_u32x4* out = (jg_u32x4*)a.out;
  auto lo = [](uint64_t x) { return (uint32_t)x; };
  auto hi = [](uint64_t x) { return (uint32_t)(x >> 32); };
#pragma unroll
  for (uint32_t k = 0; k < JG_CMT_ROWS; k++) {
    uint32_t before = 0, row = 0;
#pragma unroll
    for (uint32_t x = 0; x < JG_BLOCK / 64; x++) {
      before += x < wave ? wave_n[k][x] : 0u;
      row += wave_n[k][x];
    }
    const uint64_t pos = base + before + __popcll(m[k] & below);
    if (((m[k] >> lane) & 1ull) && pos < a.cap) {
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
    }
    base += row;
  }
}

// one workgroup: wave x reduces words x, x + 4, ... over the partial records, its lanes side by side over the records
__global__ __launch_bounds__(JG_BLOCK) void k_commit_backlog_sum(JgCommitArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t x = wave; x < JG_CMT_WORDS; x += JG_BLOCK / 64) {  // (uniform over the wave)
    uint64_t t = 0;
    for (uint32_t b = lane; b < a.parts; b += 64) t += a.part[(size_t)b * JG_CMT_WORDS + x];
    t = jg_wave_sum64(t);
    if (lane == 0) a.sum[x] = t;
  }
}
