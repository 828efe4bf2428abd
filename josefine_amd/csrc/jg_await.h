// jg_await.h — gfx950 kernels of jg_engine_watch_completions: the completion feed, fsm::Driver's notifications
// (src/raft/fsm.rs:35, 56-84) as a table of waiters in device memory.  A WAITER is 48 bytes in three 16-byte pieces
// {group, flags, token} {block_id, term} {deadline_ms, reserved}; the table keeps them in registration order, in one of two
// buffers.  A watch decides every waiter's VERDICT from its slot's columns as jg_read_state returns them (the commit
// decoded with jg_read_commit, as the commit feed and the point queries do), delivers the first `cap` done waiters in
// table order and compacts the survivors, order kept, into the other buffer.
//
// Each pass is ONE body over the resolved table - tab[0 .. n), the other buffer `dst` - and its kernels are wrappers that
// resolve that view and call it: the synchronous watch's from the host's n and cur in the arguments, an awaited step's (the
// _kept kernels, below) from the table's head on the device, behind the step's gate.
//
//   the count pass     jg_await_count_tiles (k_await_count, k_await_count_kept): one lane per waiter, a tile of JG_AWT_TILE
//                      waiters at a time: the waiter as three 16-byte loads, then its slot's columns as a gather in the
//                      manner of k_lookup - the flag word, term, head, mlag, commit, run_hi, all issued before the first use
//                      (one round trip; 44 bytes used of six 64-byte sectors) - the verdict byte stored, "done" counted by
//                      one 64-bit __ballot and a __popcll per wave, the wave counts into the tile count (jg_tile_count,
//                      jg_compact.h).  A workgroup takes the tiles b, b + grid, ..., so there are at most JG_AWT_PARTS
//                      partial stat records (jg_block_words; counts by ballots: exact in any order).  A tile wholly beyond
//                      n counts 0: an awaited step is launched for the host's bound on n, which the table may not reach
//   k_scan_block_sums  (jg_sparse.h) the tile counts -> exclusive prefixes and the total
//   k_await_stats_sum  the partial records -> the stats (jg_parts_reduce: one workgroup)
//   the write pass     jg_await_write_tile (k_await_write, k_await_write_kept), a workgroup per tile: reads verdict and
//                      prefix: the rank among the done = the rank in the tile (jg_rank_in_tile) + the tile prefix.  Done and
//                      rank < cap: DELIVERED - the slot's columns gathered again (for delivered rows only: the count pass
//                      keeps no side record) and the row written as three 16-byte stores.  Else, unless peeking, the waiter
//                      is copied to position i - min(rank, cap) of the other buffer: one scan serves both ranks.  Nothing
//                      to deliver (the total is 0, or cap is): every workgroup returns after its first load; a tile wholly
//                      beyond n returns too
//
//   the mark pass      jg_await_mark_tiles (k_await_mark, k_await_mark_kept), jg_engine_await_cancel (ABI v24): one lane per
//                      waiter over piece 0 only - `token & mask` searched in the call's sorted keys (in LDS up to
//                      JG_AWT_KEYS_LDS of them, else in device memory), a match that
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

// the table's head on the device, for the chain of an awaited step (below): the waiters outstanding and the buffer they are in
struct JgAwaitHead {
  uint32_t n, cur, pad[2];
};
static_assert(sizeof(JgAwaitHead) == 16, "the table's head is one 16-byte record");

// The arguments of every kernel of the feed, one record for both chains (await_bind, jg_api_await.h).  After each field, who
// reads it: C the count pass, W the write pass, M the mark pass, S the sum kernels (k_await_stats_sum, k_await_mark_sum),
// A k_await_append, H k_await_header.
struct JgAwaitArgs {
  // both chains
  uint32_t peek;          // W H  1: rows only, nothing is removed
  uint32_t tiles;         // C M  tiles of JG_AWT_TILE waiters the passes are launched for
  uint32_t parts;         // C M S H  workgroups of the count and mark passes (<= JG_AWT_PARTS)
  uint32_t n_keys;        // M H  the cancel's keys (<= JG_AWAIT_CANCEL_MAX); 0: no cancel
  uint64_t now;           // C  now_ms
  uint64_t cap;           // W H  rows the caller takes
  uint64_t mask;          // M  of a waiter's token, before the search
  uint4* buf[2];          // C W M A  the table's two buffers, [room][3] each: the waiters in registration order in one, the
                          //          survivors of a watch that removes, order kept, into the other
  uint8_t* verdict;       // C W  [n] 0: waits; else the row's JG_DONE_* bits
  uint64_t* bsum;         // C W  [tiles] the tile counts of done waiters, then (k_scan_block_sums) their exclusive prefixes
  uint64_t* part;         // C S H  [parts][JG_AWT_WORDS] the count pass's partial stat records
  const uint64_t* total;  // W H  [1] done waiters of the table (k_scan_block_sums)
  uint4* out;             // W  [cap] rows of three 16-byte pieces (device)
  const uint64_t* keys;   // M  [n_keys] sorted, distinct, every one within mask (device)
  uint64_t* mpart;        // M S H  [parts] the waiters each workgroup of the mark pass marked
  // the synchronous chain: the table's view is the host's
  uint32_t n;             // C W M  waiters outstanding: the table is buf[cur][0 .. n)
  uint32_t cur;           // C W M  the buffer they are in
  uint32_t add;           // W  added to every group written (a shard's first global slot; an awaited step's is 0)
  uint64_t* sum;          // S  [JG_AWT_WORDS] the stats
  uint64_t* marked;       // S  [1] the waiters the call marked
  // the chain of an awaited step: the table's view is the head's
  uint32_t m;             // A C W M H  staged rows, appended first
  uint32_t room;          // A C W M H  the table's capacity in waiters
  uint32_t stats;         // H  1: the stats are wanted
  JgAwaitHead* head;      // A C W M, written by H alone
  const uint32_t* gate;   // A C W M H  or null
  const uint4* rows;      // A  [m][3] the staged rows
  uint64_t* hdr;          // H  [JG_AH_WORDS] the header block
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

// The count pass over tab[0 .. n): the workgroup takes the tiles b, b + parts, ... (< tiles), one lane per waiter.  The verdict
// byte of every waiter, bsum[tile] = the tile's done waiters - 0 for a tile wholly beyond n - and part[b] = the workgroup's
// stat words.
__device__ __forceinline__ void jg_await_count_tiles(const JgDev& d, const uint4* tab, uint32_t n, uint32_t tiles, uint32_t parts, uint64_t now,
                                                     uint8_t* verdict, uint64_t* bsum, uint64_t* part) {
  const uint32_t live = n / JG_AWT_TILE + (n % JG_AWT_TILE ? 1u : 0u);  // the tiles that hold a waiter
  uint32_t bc[JG_AWT_WORDS] = {0u, 0u, 0u, 0u, 0u};  // wave-uniform (every lane adds the same popcount)
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += parts) {  // (uniform over the workgroup)
    // (uniform) a tile wholly beyond the table - launched for a bound that was not reached - counts 0 and goes on.  Through
    // the one store below: a store of its own, and the 64-bit tile * JG_AWT_TILE >= n, cost the kernels 2 VGPRs each
    uint32_t t = 0;
    if (tile < live) {
      const uint32_t i = tile * JG_AWT_TILE + threadIdx.x;
      const bool in = i < n;
      const size_t at = (size_t)(in ? i : 0u) * 3;
      const uint4 w0 = tab[at], w1 = tab[at + 1], w2 = tab[at + 2];
      const uint32_t g = w0.x < d.G ? w0.x : 0u;  // (checked at registration: never taken)
      // one round trip: the six unconditional loads of the slot, back to back
      const uint32_t f = d.flags[g];
      const uint64_t term_now = d.term[g], head = d.head[g], pw = d.mlag[g], col = d.commit[g], run_hi = d.run_hi[g];
      const uint64_t commit = jg_read_commit(d, g, f);  // (its loads are the ones above: nothing was stored since)
      // (the loads stay up there: without an unconditional use the compiler sinks one behind the branch on the role)
      asm volatile("" ::"v"(f), "v"(term_now), "v"(head), "v"(pw), "v"(col), "v"(run_hi));
      const uint32_t role = f & JGF_ROLE_MASK, fault = (f & JGF_FAULT_MASK) >> JGF_FAULT_SHIFT;
      const uint32_t v = in ? jg_await_verdict(w0.y, role, fault, term_now, commit, jg_awt_u64(w1.x, w1.y), jg_awt_u64(w1.z, w1.w),
                                               jg_awt_u64(w2.x, w2.y), now)
                            : 0u;
      if (in) verdict[i] = (uint8_t)v;
      const uint64_t m = __ballot(in && v);
      bc[0] += __popcll(__ballot(in && !v));
      bc[1] += __popcll(m);
      bc[2] += __popcll(__ballot(in && (v & JG_DONE_APPLIED)));
      bc[3] += __popcll(__ballot(in && (v & JG_DONE_LOST)));
      bc[4] += __popcll(__ballot(in && (v & JG_DONE_EXPIRED)));
      t = jg_tile_count(__popcll(m));
    }
    if (threadIdx.x == 0) bsum[tile] = t;
    __syncthreads();  // (jg_tile_count's LDS is the next tile's too)
  }
  const uint64_t vals[JG_AWT_WORDS] = {bc[0], bc[1], bc[2], bc[3], bc[4]};
  jg_block_words<JG_AWT_WORDS>(vals, JgNeverMax(), part);
}

// The write pass over tile blockIdx.x of tab[0 .. n), behind the scan: the done waiters of rank < cap as rows into `out`,
// groups + add; unless peeking, every other waiter into dst.
__device__ __forceinline__ void jg_await_write_tile(const JgDev& d, const uint4* tab, uint4* dst, uint32_t n, uint32_t add, uint32_t peek, uint64_t cap,
                                                    const uint64_t* total, const uint8_t* verdict, const uint64_t* bsum, uint4* out) {
  const uint64_t done = *total;
  if ((done < cap ? done : cap) == 0) return;  // (uniform over the launch) nothing is delivered: the table stays as it is
  if ((uint64_t)blockIdx.x * JG_AWT_TILE >= n) return;  // (uniform over the workgroup) wholly beyond the table
  const uint64_t base = bsum[blockIdx.x];
  if (peek && base >= cap) return;  // (uniform over the workgroup) a peek copies no waiter: wholly beyond cap
  const uint32_t i = blockIdx.x * JG_AWT_TILE + threadIdx.x;
  const bool in = i < n;
  const uint32_t v = in ? verdict[i] : 0u;
  const uint64_t rank = base + jg_rank_in_tile(__ballot(in && v));  // the done waiters before this one
  if (!in) return;
  const bool deliver = v && rank < cap;
  if (!deliver && peek) return;
  const size_t at = (size_t)i * 3;
  const uint4 w0 = tab[at], w1 = tab[at + 1], w2 = tab[at + 2];
  if (!deliver) {  // a survivor: behind it min(rank, cap) waiters leave
    const size_t to = ((size_t)i - (size_t)(rank < cap ? rank : cap)) * 3;
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
  // the row as three 16-byte pieces: {group, state | role | fault | self_slot, token} {block_id, term_now} {commit_now, head_now}
  jg_u32x4* row = (jg_u32x4*)out + rank * 3;
  row[0] = jg_u32x4{add + g, v | role << 8 | fault << 16 | self << 24, w0.z, w0.w};
  row[1] = jg_u32x4{w1.x, w1.y, lo(term_now), hi(term_now)};
  row[2] = jg_u32x4{lo(commit), hi(commit), lo(head), hi(head)};
}

// the synchronous watch's kernels: the table's view is the host's n and cur
__global__ __launch_bounds__(JG_BLOCK) void k_await_count(JgDev d, JgAwaitArgs a) {
  jg_await_count_tiles(d, a.buf[a.cur & 1u], a.n, a.tiles, a.parts, a.now, a.verdict, a.bsum, a.part);
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_stats_sum(JgAwaitArgs a) {
  jg_parts_reduce<JG_AWT_WORDS>(a.part, a.parts, a.sum, JgNeverMax());
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_write(JgDev d, JgAwaitArgs a) {
  const uint32_t cur = a.cur & 1u;
  jg_await_write_tile(d, a.buf[cur], a.buf[cur ^ 1u], a.n, a.add, a.peek, a.cap, a.total, a.verdict, a.bsum, a.out);
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

__global__ __launch_bounds__(JG_BLOCK) void k_await_mark(JgAwaitArgs a) {
  jg_await_mark_tiles(a.buf[a.cur & 1u], a.n, a.tiles, a.parts, a.keys, a.n_keys, a.mask, a.mpart);
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_mark_sum(JgAwaitArgs a) {
  jg_parts_reduce<1>(a.mpart, a.parts, a.marked, JgNeverMax());
}

// ---- the feed behind a kept node step (jg_step_node_awaited) --------------------------------------------------------------
// With kept steps outstanding the host knows neither how many waiters the table holds nor which buffer holds them: both are
// the outcome of watches whose totals have not come home.  So the table has a HEAD on the device, {n, cur}, and the chain
// of an awaited step reads it there:
//
//   k_await_append      the step's m staged rows (its arena's, uploaded behind the step) to buf[cur] + n * 3: one 16-byte
//                       piece a lane, consecutive lanes consecutive pieces; the head read once per workgroup, never written
//   k_await_mark_kept   (the step carries a cancel) the mark, count and write passes as above.  What these wrappers add: the
//   k_await_count_kept  gate, and the view - n_eff = head.n + m waiters of buf[head.cur], so rows the same step registered can
//   k_await_write_kept  be withdrawn by it.  Launched for the host's BOUND on n_eff (`tiles`): the passes leave a tile wholly
//                       beyond n_eff alone, so the one scan over `tiles` holds.  Rows are delivered with add = 0
//   k_await_header      one workgroup behind them: the partial stat records folded (k_await_stats_sum's job) and the mark
//                       pass's partials (k_await_mark_sum's), the answer but the rows as ONE block - and then, alone of
//                       the chain, the head: n = n_eff - removed, cur flipped if something was removed.  Every kernel
//                       before it read the same head
//
// `gate` is the step's general-row count on the device (null: no gate), one scalar load per workgroup: nonzero, and the
// whole chain leaves table, head and rows alone - the header block says so - for the same request is queued once more,
// ungated, behind the step's catch-up pass.  An append that ran in both would register every waiter twice.

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

__device__ __forceinline__ bool jg_await_gated(const uint32_t* gate) { return gate && *gate; }
// the waiters of the table once the step's rows are behind them; never beyond the room (the host's bound keeps it so)
__device__ __forceinline__ uint32_t jg_await_n_eff(const JgAwaitArgs& a, uint32_t n) {
  const uint64_t e = (uint64_t)n + a.m;
  return e > a.room ? a.room : (uint32_t)e;
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_append(JgAwaitArgs a) {
  if (jg_await_gated(a.gate)) return;
  const uint32_t n = a.head->n, cur = a.head->cur & 1u;  // (uniform: once per workgroup)
  if ((uint64_t)n + a.m > a.room) return;                // (never taken: refused by the host's bound)
  const size_t i = (size_t)blockIdx.x * JG_BLOCK + threadIdx.x;
  if (i < (size_t)a.m * 3) a.buf[cur][(size_t)n * 3 + i] = a.rows[i];
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_mark_kept(JgAwaitArgs a) {
  if (jg_await_gated(a.gate)) return;
  jg_await_mark_tiles(a.buf[a.head->cur & 1u], jg_await_n_eff(a, a.head->n), a.tiles, a.parts, a.keys, a.n_keys, a.mask, a.mpart);
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_count_kept(JgDev d, JgAwaitArgs a) {
  if (jg_await_gated(a.gate)) return;
  jg_await_count_tiles(d, a.buf[a.head->cur & 1u], jg_await_n_eff(a, a.head->n), a.tiles, a.parts, a.now, a.verdict, a.bsum, a.part);
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_write_kept(JgDev d, JgAwaitArgs a) {
  if (jg_await_gated(a.gate)) return;
  const uint32_t cur = a.head->cur & 1u;
  jg_await_write_tile(d, a.buf[cur], a.buf[cur ^ 1u], jg_await_n_eff(a, a.head->n), 0u, a.peek, a.cap, a.total, a.verdict, a.bsum, a.out);
}

__global__ __launch_bounds__(JG_BLOCK) void k_await_header(JgAwaitArgs a) {
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
