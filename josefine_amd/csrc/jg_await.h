// jg_await.h — gfx950 kernels of jg_engine_watch_completions: the completion feed, fsm::Driver's notifications
// (src/raft/fsm.rs:35, 56-84) as a table of waiters in device memory.  A WAITER is 48 bytes in three 16-byte pieces
// {group, flags, token} {block_id, term} {deadline_ms, reserved}; the table keeps them in registration order, in one of two
// buffers.  A watch decides every waiter's VERDICT from its slot's columns as jg_read_state returns them (the commit
// decoded with jg_read_commit, as the commit feed and the point queries do), delivers the first `cap` done waiters in
// table order and compacts the survivors, order kept, into the other buffer.
//
//   k_await_count      one lane per waiter, a tile of JG_AWT_TILE waiters at a time: the waiter as three 16-byte loads,
//                      then its slot's columns as a gather in the manner of k_lookup - the flag word, term, head, mlag,
//                      commit, run_hi, all issued before the first use (one round trip; 44 bytes used of six 64-byte
//                      sectors) - the verdict byte stored, "done" counted by one 64-bit __ballot and a __popcll per wave,
//                      the wave counts into the tile count (jg_tile_count, jg_compact.h).  A workgroup takes the tiles
//                      b, b + grid, ..., so there are at most JG_AWT_PARTS partial stat records (jg_block_words; counts by
//                      ballots: exact in any order)
//   k_scan_block_sums  (jg_sparse.h) the tile counts -> exclusive prefixes and the total
//   k_await_stats_sum  the partial records -> the stats (jg_parts_reduce: one workgroup)
//   k_await_write      reads verdict and prefix: the rank among the done = the rank in the tile (jg_rank_in_tile) + the
//                      tile prefix.  Done and rank < cap: DELIVERED - the slot's columns gathered again (for delivered rows
//                      only: the count pass keeps no side record) and the row written as three 16-byte stores.  Else,
//                      unless peeking, the waiter is copied to position i - min(rank, cap) of the other buffer: one scan
//                      serves both ranks.  Nothing to deliver (the total is 0, or cap is): every workgroup returns after
//                      its first load
//
//   k_await_mark       jg_engine_await_cancel (ABI v24): one lane per waiter over piece 0 only - `token & mask` searched in
//                      the call's sorted keys (in LDS up to JG_AWT_KEYS_LDS of them, else in device memory), a match that
//                      is not marked yet gets JG_AWAIT_WITHDRAWN into its flag word, in place: the one store to the table
//                      (4 bytes).  The newly marked counted by ballots into one partial per workgroup, folded by
//                      k_await_mark_sum.  A marked waiter's verdict is JG_DONE_CANCELLED whatever its slot looks like
//                      (rule 0 of jg_await_verdict); it leaves at the next watch as every done waiter does
//
// No atomics, no scratch.  Nothing here writes a column of the state machine: the only stores are the verdict bytes, the
// tile counts, the partial records, the rows, the other buffer and the marks.
#pragma once
#include "jg_device.h"
#include "jg_lookup.h"  // jg_u32x4
#include "jg_read.h"    // jg_read_commit
#include "jg_sparse.h"  // JgScanJob, k_scan_block_sums
#include "jg_compact.h"

#define JG_AWT_TILE JG_BLOCK  // waiters per tile of the passes: one lane per waiter
// the most workgroups - partial stat records - of the count pass: four a CU on 256 CUs (JG_CMT_PARTS)
#define JG_AWT_PARTS 1024u
#define JG_AWT_WORDS 5u  // waiting, done, applied, lost, expired: the first five words of jg_await_stats (`left` is the host's)
static_assert(sizeof(jg_await_stats) == (JG_AWT_WORDS + 1) * 8, "jg_await_stats is the stat words in order, then left");
static_assert(sizeof(jg_await_row) == 48, "jg_await_row is three 16-byte pieces");
static_assert(sizeof(jg_done_row) == 48, "jg_done_row is three 16-byte pieces");

struct JgAwaitArgs {
  uint32_t n;      // waiters outstanding: the table is tab[0 .. n)
  uint32_t add;    // added to every group written (a shard's first global slot)
  uint32_t peek;   // 1: rows only, nothing is removed
  uint32_t tiles;  // tiles of JG_AWT_TILE waiters
  uint32_t parts;  // workgroups of k_await_count (<= JG_AWT_PARTS)
  uint32_t pad;
  uint64_t now;           // now_ms
  uint64_t cap;           // rows the caller takes
  const uint4* tab;       // [n][3] the waiters, registration order
  uint4* dst;             // [n][3] the other buffer: the survivors, order kept
  uint8_t* verdict;       // [n] 0: waits; else the row's JG_DONE_* bits
  uint64_t* bsum;         // [tiles] the tile counts of done waiters, then (k_scan_block_sums) their exclusive prefixes
  uint64_t* part;         // [parts][JG_AWT_WORDS]
  uint64_t* sum;          // [JG_AWT_WORDS] the stats
  const uint64_t* total;  // [1] done waiters of the table (k_scan_block_sums)
  uint4* out;             // [cap] rows of three 16-byte pieces (device)
};

__device__ __forceinline__ uint64_t jg_awt_u64(uint32_t lo, uint32_t hi) { return (uint64_t)lo | (uint64_t)hi << 32; }

// The verdict of a waiter (flags, block_id, term, deadline) on a slot in (role, fault, term_now, commit): the first rule wins.
//   0. withdrawn (jg_engine_await_cancel marked it) -> CANCELLED, whatever the slot looks like
//   1. vacant -> LOST | VACANT; any other fault -> LOST | FAULTED
//   2. a guarded waiter (term != 0) whose slot is not the leader of that term any more -> LOST.  Before the applied test on
//      purpose: a block that committed under a later leadership cannot be told from a different block with the same id
//   3. applied - the two key conventions of the commit feed from genesis: a leader's Apply keys are (.., commit], a
//      follower's [.., commit)
//   4. past its deadline -> EXPIRED
__device__ __forceinline__ uint32_t jg_await_verdict(uint32_t wflags, uint32_t role, uint32_t fault, uint64_t term_now, uint64_t commit,
                                                     uint64_t block_id, uint64_t term, uint64_t deadline, uint64_t now) {
  if (wflags & JG_AWAIT_WITHDRAWN) return JG_DONE_CANCELLED;
  if (fault == JG_FAULT_VACANT) return JG_DONE_LOST | JG_DONE_VACANT;
  if (fault) return JG_DONE_LOST | JG_DONE_FAULTED;
  const bool leads = role == JG_ROLE_LEADER;
  if (term && (!leads || term_now != term)) return JG_DONE_LOST;
  if (leads ? block_id <= commit : block_id < commit) return JG_DONE_APPLIED;
  if (deadline && now >= deadline) return JG_DONE_EXPIRED;
  return 0u;
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_count(JgDev d, JgAwaitArgs a) {
  uint32_t bc[JG_AWT_WORDS] = {0u, 0u, 0u, 0u, 0u};  // wave-uniform (every lane adds the same popcount)
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += a.parts) {  // (uniform over the workgroup)
    const uint32_t i = tile * JG_AWT_TILE + threadIdx.x;
    const bool in = i < a.n;
    const size_t at = (size_t)(in ? i : 0u) * 3;
    const uint4 w0 = a.tab[at], w1 = a.tab[at + 1], w2 = a.tab[at + 2];
    const uint32_t g = w0.x < d.G ? w0.x : 0u;  // (checked at registration: never taken)
    // one round trip: the six unconditional loads of the slot, back to back
    const uint32_t f = d.flags[g];
    const uint64_t term_now = d.term[g], head = d.head[g], pw = d.mlag[g], col = d.commit[g], run_hi = d.run_hi[g];
    const uint64_t commit = jg_read_commit(d, g, f);  // (its loads are the ones above: nothing was stored since)
    // (the loads stay up there: without an unconditional use the compiler sinks one behind the branch on the role)
    asm volatile("" ::"v"(f), "v"(term_now), "v"(head), "v"(pw), "v"(col), "v"(run_hi));
    const uint32_t role = f & JGF_ROLE_MASK, fault = (f & JGF_FAULT_MASK) >> JGF_FAULT_SHIFT;
    const uint32_t v = in ? jg_await_verdict(w0.y, role, fault, term_now, commit, jg_awt_u64(w1.x, w1.y), jg_awt_u64(w1.z, w1.w),
                                             jg_awt_u64(w2.x, w2.y), a.now)
                          : 0u;
    if (in) a.verdict[i] = (uint8_t)v;
    const uint64_t m = __ballot(in && v);
    bc[0] += __popcll(__ballot(in && !v));
    bc[1] += __popcll(m);
    bc[2] += __popcll(__ballot(in && (v & JG_DONE_APPLIED)));
    bc[3] += __popcll(__ballot(in && (v & JG_DONE_LOST)));
    bc[4] += __popcll(__ballot(in && (v & JG_DONE_EXPIRED)));
    const uint32_t t = jg_tile_count(__popcll(m));
    if (threadIdx.x == 0) a.bsum[tile] = t;
    __syncthreads();  // (jg_tile_count's LDS is the next tile's too)
  }
  const uint64_t vals[JG_AWT_WORDS] = {bc[0], bc[1], bc[2], bc[3], bc[4]};
  jg_block_words<JG_AWT_WORDS>(vals, JgNeverMax(), a.part);
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_stats_sum(JgAwaitArgs a) {
  jg_parts_reduce<JG_AWT_WORDS>(a.part, a.parts, a.sum, JgNeverMax());
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_write(JgDev d, JgAwaitArgs a) {
  const uint64_t total = *a.total;
  if ((total < a.cap ? total : a.cap) == 0) return;  // (uniform over the launch) nothing is delivered: the table stays as it is
  const uint64_t base = a.bsum[blockIdx.x];
  if (a.peek && base >= a.cap) return;  // (uniform over the workgroup) a peek copies no waiter: wholly beyond cap
  const uint32_t i = blockIdx.x * JG_AWT_TILE + threadIdx.x;
  const bool in = i < a.n;
  const uint32_t v = in ? a.verdict[i] : 0u;
  const uint64_t rank = base + jg_rank_in_tile(__ballot(in && v));  // the done waiters before this one
  if (!in) return;
  const bool deliver = v && rank < a.cap;
  if (!deliver && a.peek) return;
  const size_t at = (size_t)i * 3;
  const uint4 w0 = a.tab[at], w1 = a.tab[at + 1], w2 = a.tab[at + 2];
  if (!deliver) {  // a survivor: behind it min(rank, cap) waiters leave
    const size_t to = ((size_t)i - (size_t)(rank < a.cap ? rank : a.cap)) * 3;
    a.dst[to] = w0, a.dst[to + 1] = w1, a.dst[to + 2] = w2;
    return;
  }
  const uint32_t g = w0.x < d.G ? w0.x : 0u;
  const uint32_t f = d.flags[g];
  const uint64_t term_now = d.term[g], head = d.head[g];
  const uint64_t commit = jg_read_commit(d, g, f);
  const uint32_t role = f & JGF_ROLE_MASK, fault = (f & JGF_FAULT_MASK) >> JGF_FAULT_SHIFT, self = (f & JGF_SELF_MASK) >> JGF_SELF_SHIFT;
  auto lo = [](uint64_t x) { return (uint32_t)x; };
  auto hi = [](uint64_t x) { return (uint32_t)(x >> 32); };
  // the row as three 16-byte pieces: {group, state | role | fault | self_slot, token} {block_id, term_now} {commit_now, head_now}
  jg_u32x4* out = (jg_u32x4*)a.out + rank * 3;
  out[0] = jg_u32x4{a.add + g, v | role << 8 | fault << 16 | self << 24, w0.z, w0.w};
  out[1] = jg_u32x4{w1.x, w1.y, lo(term_now), hi(term_now)};
  out[2] = jg_u32x4{lo(commit), hi(commit), lo(head), hi(head)};
}

// ---- withdrawing waiters (jg_engine_await_cancel) ---------------------------------------------------------------------------
#define JG_AWT_KEYS_LDS 2048u  // the keys a workgroup stages into LDS (16 KB); more are searched in device memory (L2)

// key among the sorted, distinct keys[0 .. n)?  (a lower bound by halving: at most 17 probes for JG_AWAIT_CANCEL_MAX keys)
__device__ __forceinline__ bool jg_awt_has_key(const uint64_t* keys, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && keys[lo] == key;
}

// The mark pass over tab[0 .. n): the workgroup takes the tiles b, b + parts, ... (< tiles; a tile wholly beyond n ends it),
// one lane per waiter, piece 0 only.  A waiter whose token & mask is among the keys and that is not marked yet gets the mark
// into its flag word - a 4-byte store, the only one to the table.  part[b] = the waiters this workgroup marked.
__device__ __forceinline__ void jg_await_mark_tiles(uint4* tab, uint32_t n, uint32_t tiles, uint32_t parts, const uint64_t* keys, uint32_t n_keys,
                                                    uint64_t mask, uint64_t* part) {
  __shared__ uint64_t lds_keys[JG_AWT_KEYS_LDS];
  const bool staged = n_keys <= JG_AWT_KEYS_LDS;  // (uniform over the launch)
  if (staged) {  // once, before the first tile: consecutive lanes, consecutive keys
    for (uint32_t k = threadIdx.x; k < n_keys; k += JG_BLOCK) lds_keys[k] = keys[k];
    __syncthreads();
  }
  uint32_t marked = 0;  // wave-uniform (every lane adds the same popcount)
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += parts) {  // (uniform over the workgroup)
    if ((uint64_t)tile * JG_AWT_TILE >= n) break;
    const uint32_t i = tile * JG_AWT_TILE + threadIdx.x;
    const bool in = i < n;
    const size_t at = (size_t)(in ? i : 0u) * 3;
    const uint4 w0 = tab[at];
    const uint64_t key = jg_awt_u64(w0.z, w0.w) & mask;
    const bool has = staged ? jg_awt_has_key(lds_keys, n_keys, key) : jg_awt_has_key(keys, n_keys, key);
    const bool hit = in && has && !(w0.y & JG_AWAIT_WITHDRAWN);
    if (hit) ((uint32_t*)(tab + at))[1] = w0.y | JG_AWAIT_WITHDRAWN;
    marked += __popcll(__ballot(hit));
  }
  const uint64_t vals[1] = {marked};
  jg_block_words<1>(vals, JgNeverMax(), part);
}

struct JgAwaitMarkArgs {
  uint32_t n;       // waiters outstanding: the table is tab[0 .. n)
  uint32_t tiles;   // tiles of JG_AWT_TILE waiters
  uint32_t parts;   // workgroups (<= JG_AWT_PARTS)
  uint32_t n_keys;  // <= JG_AWAIT_CANCEL_MAX
  uint64_t mask;
  uint4* tab;            // [n][3] the waiters
  const uint64_t* keys;  // [n_keys] sorted, distinct, every one within mask (device)
  uint64_t* part;        // [parts] the waiters each workgroup marked
  uint64_t* sum;         // [1] the waiters the call marked
};

__global__ __launch_bounds__(JG_BLOCK) void k_await_mark(JgAwaitMarkArgs a) {
  jg_await_mark_tiles(a.tab, a.n, a.tiles, a.parts, a.keys, a.n_keys, a.mask, a.part);
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_mark_sum(JgAwaitMarkArgs a) {
  jg_parts_reduce<1>(a.part, a.parts, a.sum, JgNeverMax());
}

// ---- the feed behind a kept node step (jg_step_node_awaited) --------------------------------------------------------------
// With kept steps outstanding the host knows neither how many waiters the table holds nor which buffer holds them: both are
// the outcome of watches whose totals have not come home.  So the table has a HEAD on the device, {n, cur}, and the chain
// of an awaited step reads it there:
//
//   k_await_append      the step's m staged rows (its arena's, uploaded behind the step) to buf[cur] + n * 3: one 16-byte
//                       piece a lane, consecutive lanes consecutive pieces; the head read once per workgroup, never written
//   k_await_mark_kept   (the step carries a cancel) the mark pass over n_eff = head.n + m waiters of buf[head.cur]: rows the
//                       same step registered can be withdrawn by it
//   k_await_count_kept  k_await_count over n_eff = head.n + m waiters of buf[head.cur], launched for the host's BOUND on
//   k_await_write_kept  n_eff (`tiles`); a tile wholly beyond n_eff counts 0 / returns, so the one scan over `tiles` holds
//   k_await_header      one workgroup behind them: the partial stat records folded (k_await_stats_sum's job) and the mark
//                       pass's partials (k_await_mark_sum's), the answer but
//                       the rows as ONE block - and then, alone of the chain, the head: n = n_eff - removed, cur flipped if
//                       something was removed.  Every kernel before it read the same head
//
// `gate` is the step's general-row count on the device (null: no gate), one scalar load per workgroup: nonzero, and the
// whole chain leaves table, head and rows alone - the header block says so - for the same request is queued once more,
// ungated, behind the step's catch-up pass.  An append that ran in both would register every waiter twice.
struct JgAwaitHead {
  uint32_t n, cur, pad[2];
};
static_assert(sizeof(JgAwaitHead) == 16, "the table's head is one 16-byte record");

// the header block of an awaited step, 8-byte words
#define JG_AH_TOTAL 0u    // the done waiters
#define JG_AH_GIVEN 1u    // min(cap, total): the rows delivered
#define JG_AH_STATS 2u    // [JG_AWT_WORDS] the stats before the delivery (zero unless wanted)
#define JG_AH_LEFT (JG_AH_STATS + JG_AWT_WORDS)  // the waiters outstanding behind the call
#define JG_AH_N (JG_AH_LEFT + 1u)                // the head as this pass leaves it
#define JG_AH_CUR (JG_AH_N + 1u)
#define JG_AH_GATE (JG_AH_CUR + 1u)              // the gate's verdict: the step's general-path rows as this pass saw them
#define JG_AH_MARKED (JG_AH_GATE + 1u)            // the waiters the step's cancel marked
#define JG_AH_WORDS (JG_AH_MARKED + 1u)

struct JgAwaitKeptArgs {
  uint32_t m;       // staged rows, appended first
  uint32_t room;    // the table's capacity in waiters
  uint32_t peek;    // 1: rows only, nothing is removed
  uint32_t tiles;   // tiles of JG_AWT_TILE waiters of the host's bound on n_eff
  uint32_t parts;   // workgroups of the count pass (<= JG_AWT_PARTS)
  uint32_t stats;   // 1: the stats are wanted
  uint64_t now;     // now_ms
  uint64_t cap;     // rows the caller takes
  JgAwaitHead* head;
  const uint32_t* gate;  // or null
  const uint4* rows;     // [m][3] the staged rows
  uint4* buf[2];         // the table's two buffers
  uint8_t* verdict;
  uint64_t* bsum;         // [tiles]
  uint64_t* part;         // [parts][JG_AWT_WORDS]
  const uint64_t* total;  // [1] (k_scan_block_sums)
  uint4* out;             // [cap] rows of three 16-byte pieces (device)
  uint64_t* hdr;          // [JG_AH_WORDS]
  const uint64_t* keys;   // [n_keys] the step's cancel: sorted, distinct, every one within mask (staged behind the rows)
  uint64_t* mpart;        // [parts] the waiters each workgroup of the mark pass marked
  uint64_t mask;
  uint32_t n_keys;        // 0: the step carries no cancel
  uint32_t pad;
};

__device__ __forceinline__ bool jg_await_gated(const uint32_t* gate) { return gate && *gate; }
// the waiters of the table once the step's rows are behind them; never beyond the room (the host's bound keeps it so)
__device__ __forceinline__ uint32_t jg_await_n_eff(const JgAwaitKeptArgs& a, uint32_t n) {
  const uint64_t e = (uint64_t)n + a.m;
  return e > a.room ? a.room : (uint32_t)e;
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_append(JgAwaitKeptArgs a) {
  if (jg_await_gated(a.gate)) return;
  const uint32_t n = a.head->n, cur = a.head->cur & 1u;  // (uniform: once per workgroup)
  if ((uint64_t)n + a.m > a.room) return;                // (never taken: refused by the host's bound)
  const size_t i = (size_t)blockIdx.x * JG_BLOCK + threadIdx.x;
  if (i < (size_t)a.m * 3) a.buf[cur][(size_t)n * 3 + i] = a.rows[i];
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_mark_kept(JgAwaitKeptArgs a) {
  if (jg_await_gated(a.gate)) return;
  jg_await_mark_tiles(a.buf[a.head->cur & 1u], jg_await_n_eff(a, a.head->n), a.tiles, a.parts, a.keys, a.n_keys, a.mask, a.mpart);
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_count_kept(JgDev d, JgAwaitKeptArgs a) {
  if (jg_await_gated(a.gate)) return;
  const uint32_t n = jg_await_n_eff(a, a.head->n);
  const uint4* tab = a.buf[a.head->cur & 1u];
  uint32_t bc[JG_AWT_WORDS] = {0u, 0u, 0u, 0u, 0u};  // wave-uniform (every lane adds the same popcount)
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += a.parts) {  // (uniform over the workgroup)
    if ((uint64_t)tile * JG_AWT_TILE >= n) {  // (uniform) wholly beyond the table: the bound was not reached
      if (threadIdx.x == 0) a.bsum[tile] = 0;
      continue;
    }
    const uint32_t i = tile * JG_AWT_TILE + threadIdx.x;
    const bool in = i < n;
    const size_t at = (size_t)(in ? i : 0u) * 3;
    const uint4 w0 = tab[at], w1 = tab[at + 1], w2 = tab[at + 2];
    const uint32_t g = w0.x < d.G ? w0.x : 0u;  // (checked at registration: never taken)
    const uint32_t f = d.flags[g];
    const uint64_t term_now = d.term[g], head = d.head[g], pw = d.mlag[g], col = d.commit[g], run_hi = d.run_hi[g];
    const uint64_t commit = jg_read_commit(d, g, f);
    asm volatile("" ::"v"(f), "v"(term_now), "v"(head), "v"(pw), "v"(col), "v"(run_hi));  // (as in k_await_count: one round trip)
    const uint32_t role = f & JGF_ROLE_MASK, fault = (f & JGF_FAULT_MASK) >> JGF_FAULT_SHIFT;
    const uint32_t v = in ? jg_await_verdict(w0.y, role, fault, term_now, commit, jg_awt_u64(w1.x, w1.y), jg_awt_u64(w1.z, w1.w),
                                             jg_awt_u64(w2.x, w2.y), a.now)
                          : 0u;
    if (in) a.verdict[i] = (uint8_t)v;
    const uint64_t m = __ballot(in && v);
    bc[0] += __popcll(__ballot(in && !v));
    bc[1] += __popcll(m);
    bc[2] += __popcll(__ballot(in && (v & JG_DONE_APPLIED)));
    bc[3] += __popcll(__ballot(in && (v & JG_DONE_LOST)));
    bc[4] += __popcll(__ballot(in && (v & JG_DONE_EXPIRED)));
    const uint32_t t = jg_tile_count(__popcll(m));
    if (threadIdx.x == 0) a.bsum[tile] = t;
    __syncthreads();  // (jg_tile_count's LDS is the next tile's too)
  }
  const uint64_t vals[JG_AWT_WORDS] = {bc[0], bc[1], bc[2], bc[3], bc[4]};
  jg_block_words<JG_AWT_WORDS>(vals, JgNeverMax(), a.part);
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_write_kept(JgDev d, JgAwaitKeptArgs a) {
  if (jg_await_gated(a.gate)) return;
  const uint64_t total = *a.total;
  if ((total < a.cap ? total : a.cap) == 0) return;  // (uniform over the launch) nothing is delivered: the table stays as it is
  const uint32_t n = jg_await_n_eff(a, a.head->n), cur = a.head->cur & 1u;
  if ((uint64_t)blockIdx.x * JG_AWT_TILE >= n) return;  // (uniform over the workgroup) wholly beyond the table
  const uint64_t base = a.bsum[blockIdx.x];
  if (a.peek && base >= a.cap) return;  // (uniform over the workgroup) a peek copies no waiter: wholly beyond cap
  const uint4* tab = a.buf[cur];
  uint4* dst = a.buf[cur ^ 1u];
  const uint32_t i = blockIdx.x * JG_AWT_TILE + threadIdx.x;
  const bool in = i < n;
  const uint32_t v = in ? a.verdict[i] : 0u;
  const uint64_t rank = base + jg_rank_in_tile(__ballot(in && v));  // the done waiters before this one
  if (!in) return;
  const bool deliver = v && rank < a.cap;
  if (!deliver && a.peek) return;
  const size_t at = (size_t)i * 3;
  const uint4 w0 = tab[at], w1 = tab[at + 1], w2 = tab[at + 2];
  if (!deliver) {  // a survivor: behind it min(rank, cap) waiters leave
    const size_t to = ((size_t)i - (size_t)(rank < a.cap ? rank : a.cap)) * 3;
    dst[to] = w0, dst[to + 1] = w1, dst[to + 2] = w2;
    return;
  }
  const uint32_t g = w0.x < d.G ? w0.x : 0u;
  const uint32_t f = d.flags[g];
  const uint64_t term_now = d.term[g], head = d.head[g];
  const uint64_t commit = jg_read_commit(d, g, f);
  const uint32_t role = f & JGF_ROLE_MASK, fault = (f & JGF_FAULT_MASK) >> JGF_FAULT_SHIFT, self = (f & JGF_SELF_MASK) >> JGF_SELF_SHIFT;
  auto lo = [](uint64_t x) { return (uint32_t)x; };
  auto hi = [](uint64_t x) { return (uint32_t)(x >> 32); };
  jg_u32x4* out = (jg_u32x4*)a.out + rank * 3;  // (the row of k_await_write)
  out[0] = jg_u32x4{g, v | role << 8 | fault << 16 | self << 24, w0.z, w0.w};
  out[1] = jg_u32x4{w1.x, w1.y, lo(term_now), hi(term_now)};
  out[2] = jg_u32x4{lo(commit), hi(commit), lo(head), hi(head)};
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_header(JgAwaitKeptArgs a) {
  const uint32_t gate = a.gate ? *a.gate : 0u;
  if (gate) {  // (uniform) the pass left everything alone
    if (threadIdx.x < JG_AH_WORDS) a.hdr[threadIdx.x] = threadIdx.x == JG_AH_GATE ? gate : 0ull;
    return;
  }
  if (a.stats) jg_parts_reduce<JG_AWT_WORDS>(a.part, a.parts, a.hdr + JG_AH_STATS, JgNeverMax());
  else if (threadIdx.x < JG_AWT_WORDS) a.hdr[JG_AH_STATS + threadIdx.x] = 0;
  if (a.n_keys) jg_parts_reduce<1>(a.mpart, a.parts, a.hdr + JG_AH_MARKED, JgNeverMax());
  else if (threadIdx.x == 0) a.hdr[JG_AH_MARKED] = 0;
  if (threadIdx.x) return;
  const uint32_t n = jg_await_n_eff(a, a.head->n), cur = a.head->cur & 1u;
  const uint64_t total = *a.total, given = total < a.cap ? total : a.cap;
  const uint32_t removed = a.peek ? 0u : (uint32_t)given;
  a.hdr[JG_AH_TOTAL] = total, a.hdr[JG_AH_GIVEN] = given;
  a.hdr[JG_AH_LEFT] = a.hdr[JG_AH_N] = n - removed;
  a.hdr[JG_AH_CUR] = removed ? cur ^ 1u : cur;
  a.hdr[JG_AH_GATE] = 0;
  a.head->n = n - removed, a.head->cur = removed ? cur ^ 1u : cur;
}
