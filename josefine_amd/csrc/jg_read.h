// jg_read.h — gfx950 kernels of jg_engine_read_chains: each group's chain read back out as the rows of a sled scan
// (Chain::range(from..), chain.rs:208-228), the inverse of jg_load.h.  A group is decoded from its columns - the run
// [0, run_hi] (implicit in RUN / FAST form, absent under JGF_NO_GENESIS), up to JG_CHAIN_WINDOW window segments stored
// in any order (jg_chain_normalize swap-removes), a leader's commit lag-packed in mlag - by one thread, in registers.
// No thread and no wave walks a group's rows: a group of 10^6 blocks is one segment of the table and 10^6 rows of the
// flat row pass like any other.
//
//   k_read_groups      per group: decode, clip at from[i], commit / has_commit / fault; tile sums of rows and segments
//   k_scan_block_sums  (jg_sparse.h) both tile sums -> exclusive prefixes, one job each
//   k_read_segs        per group: decode again, the prefixes -> off[i] and the group's segments, sorted by first id, as
//                      (first id, first parent, first row) rows of the segment table
//   k_read_rows        per piece of JG_READ_PIECE rows: a thread finds the segment of its first row by one binary
//                      search, makes JG_READ_ITEMS consecutive rows (id = lo + k, next = id - 1, the first row of a
//                      segment its stored parent) into LDS, and the workgroup stores the tile as coalesced columns
#pragma once
#include "jg_device.h"
#include "jg_sparse.h"  // jg_block_exclusive_scan, JgScanJob, k_scan_block_sums

#define JG_READ_ITEMS 8u                           // rows per thread of k_read_rows
#define JG_READ_TILE (JG_BLOCK * JG_READ_ITEMS)    // rows per workgroup of k_read_rows
#define JG_READ_PIECE (1ull << 24)                 // rows per staging piece (a multiple of JG_READ_TILE): 2 x 256 MiB staged
#define JG_READ_SEGS (1u + JG_CHAIN_WINDOW)        // the run and the window segments

struct JgReadArgs {
  uint32_t n;                // groups of this call (this shard's part)
  uint32_t g0;               // first group (shard-local numbering)
  uint64_t row_base;         // added to every off[i] written (a shard's first row in the caller's numbering)
  const uint64_t* from;      // [n] or null: rows are the block keys >= from[i]
  uint64_t* commit;          // [n] out: the "commit" key's value, 0 where absent
  uint8_t* has_commit;       // [n] out
  uint8_t* fault;            // [n] out
  uint64_t* bsum_r;          // [tiles] tile sums of the rows, then their exclusive prefixes
  uint64_t* bsum_s;          // [tiles] ... of the segments
  uint64_t* total;           // [2] rows, segments of the call
  uint64_t* off;             // [n] out: first row of each group (+ row_base)
  uint64_t* seg_lo;          // [segments] first id of each (clipped) segment
  uint64_t* seg_nx;          // [segments] its parent
  uint64_t* seg_row;         // [segments] its first row (shard-local numbering)
  uint32_t* err;             // [1] 1: a tile of JG_BLOCK groups holds 2^32 rows or more
};

// One group's chain as at most JG_READ_SEGS segments [lo, hi] (next(lo) = nx, next(id) = id - 1 above it), clipped at
// `from`: slot 0 the run, slots 1.. the window sorted by lo; only the first n are valid.  All indices are compile-time
// constants (fully unrolled): the arrays live in registers.
struct JgReadSegs {
  uint64_t lo[JG_READ_SEGS], hi[JG_READ_SEGS], nx[JG_READ_SEGS];
  bool ok[JG_READ_SEGS];
  uint32_t n;
  uint64_t rows;
};

__device__ __forceinline__ void jg_read_cx(JgReadSegs& s, uint32_t a, uint32_t b) {  // compare-exchange, valid ones first
  const bool swap = s.ok[b] && (!s.ok[a] || s.lo[b] < s.lo[a]);
  if (swap) {
    const uint64_t l = s.lo[a], h = s.hi[a], x = s.nx[a];
    const bool o = s.ok[a];
    s.lo[a] = s.lo[b], s.hi[a] = s.hi[b], s.nx[a] = s.nx[b], s.ok[a] = s.ok[b];
    s.lo[b] = l, s.hi[b] = h, s.nx[b] = x, s.ok[b] = o;
  }
}

// decode group g; returns the flag word (the fault is in it); s.n = 0 for an engine-domain fault
__device__ inline uint32_t jg_read_decode(const JgDev& d, uint32_t g, uint64_t from, JgReadSegs& s) {
  const uint32_t flags = d.flags[g];
  const uint32_t fault = (flags & JGF_FAULT_MASK) >> JGF_FAULT_SHIFT;
  const uint32_t wn = fault >= 128u ? 0u : (flags & JGF_WIN_MASK) >> JGF_WIN_SHIFT;
  const uint64_t run_hi = (flags & JGF_RUN) ? d.head[g] : d.run_hi[g];
  s.lo[0] = 0, s.hi[0] = run_hi, s.nx[0] = 0;  // genesis: next 0
  s.ok[0] = fault < 128u && !(flags & JGF_NO_GENESIS);
#pragma unroll
  for (uint32_t w = 0; w < JG_CHAIN_WINDOW; w++) {
    const bool ok = w < wn;
    const size_t at = (size_t)w * d.G + g;
    s.lo[1 + w] = ok ? d.win_lo[at] : 0;
    s.hi[1 + w] = ok ? d.win_hi[at] : 0;
    s.nx[1 + w] = ok ? d.win_next[at] : 0;
    s.ok[1 + w] = ok;
  }
  // clip at from: [lo, hi] -> [max(lo, from), hi]; a clipped first row's parent is its predecessor
#pragma unroll
  for (uint32_t k = 0; k < JG_READ_SEGS; k++) {
    if (s.hi[k] < from) s.ok[k] = false;
    if (s.lo[k] < from) s.lo[k] = from, s.nx[k] = from - 1;
  }
  // the run is below every window segment (ids are disjoint, the run starts at 0): sort the window only
  // (odd-even transposition: JG_CHAIN_WINDOW rounds of constant-index compare-exchanges)
#pragma unroll
  for (uint32_t r = 0; r < JG_CHAIN_WINDOW; r++) {
#pragma unroll
    for (uint32_t a = 1 + (r & 1u); a + 1 < JG_READ_SEGS; a += 2) jg_read_cx(s, a, a + 1);
  }
  s.n = 0;
  s.rows = 0;
#pragma unroll
  for (uint32_t k = 0; k < JG_READ_SEGS; k++)
    if (s.ok[k]) s.n++, s.rows += s.hi[k] - s.lo[k] + 1;
  return flags;
}

// Chain.commit as jg_read_state(JG_FIELD_COMMIT) decodes it: leaders keep it as field R of mlag, a lag below the chain's
// top (jg_lag_base_is_run_hi) unless the field is an escape
__device__ __forceinline__ uint64_t jg_read_commit(const JgDev& d, uint32_t g, uint32_t flags) {
  if ((flags & JGF_ROLE_MASK) != JG_ROLE_LEADER) return d.commit[g];
  const uint64_t fc = jg_lag_field(d.mlag[g], d.R, d.R);
  if (jg_lag_wide(fc, d.R)) return d.commit[g];
  return (jg_lag_base_is_run_hi(flags) ? d.run_hi[g] : d.head[g]) - fc;
}

// exclusive scan of one 64-bit value per thread across the workgroup (jg_block_exclusive_scan, 64 bits wide)
__device__ __forceinline__ uint64_t jg_block_exclusive_scan64(uint64_t v, uint64_t* total) {
  __shared__ uint64_t wave_tot64[JG_BLOCK / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t up = __shfl_up(inc, off, 64);
    if (lane >= (uint32_t)off) inc += up;
  }
  if (lane == 63) wave_tot64[wave] = inc;
  __syncthreads();
  uint64_t base = 0, tot = 0;
#pragma unroll
  for (uint32_t w = 0; w < JG_BLOCK / 64; w++) {
    base += w < wave ? wave_tot64[w] : 0ull;
    tot += wave_tot64[w];
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

__global__ __launch_bounds__(JG_BLOCK) void k_read_groups(JgDev d, JgReadArgs a) {
  const uint32_t i = blockIdx.x * JG_BLOCK + threadIdx.x;
  uint64_t rows = 0;
  uint32_t nseg = 0;
  if (i < a.n) {
    const uint32_t g = a.g0 + i;
    JgReadSegs s;
    const uint32_t flags = jg_read_decode(d, g, a.from ? a.from[i] : 0, s);
    const uint32_t fault = (flags & JGF_FAULT_MASK) >> JGF_FAULT_SHIFT;
    const bool has = fault < 128u && (flags & JGF_COMMIT_KEY);
    a.commit[i] = has ? jg_read_commit(d, g, flags) : 0;  // (the key is written with Chain.commit, chain.rs:198-199)
    a.has_commit[i] = has ? 1 : 0;
    a.fault[i] = (uint8_t)fault;
    rows = s.rows;
    nseg = s.n;
  }
  uint64_t tot_r;
  uint32_t tot_s;
  (void)jg_block_exclusive_scan64(rows, &tot_r);
  (void)jg_block_exclusive_scan(nseg, &tot_s);
  if (threadIdx.x == 0) {
    a.bsum_r[blockIdx.x] = tot_r;
    a.bsum_s[blockIdx.x] = tot_s;
    if (tot_r >> 32) atomicOr(a.err, 1u);  // (k_scan_block_sums adds the tile sums as 32-bit values)
  }
}

__global__ __launch_bounds__(JG_BLOCK) void k_read_segs(JgDev d, JgReadArgs a) {
  const uint32_t i = blockIdx.x * JG_BLOCK + threadIdx.x;
  JgReadSegs s;
  s.n = 0;
  s.rows = 0;
  if (i < a.n) (void)jg_read_decode(d, a.g0 + i, a.from ? a.from[i] : 0, s);
  uint64_t tot_r;
  uint32_t tot_s;
  uint64_t row = a.bsum_r[blockIdx.x] + jg_block_exclusive_scan64(s.rows, &tot_r);
  const uint64_t sb = a.bsum_s[blockIdx.x] + jg_block_exclusive_scan(s.n, &tot_s);
  if (i >= a.n) return;
  a.off[i] = a.row_base + row;
  uint64_t at = sb;
#pragma unroll
  for (uint32_t k = 0; k < JG_READ_SEGS; k++)
    if (s.ok[k]) {
      a.seg_lo[at] = s.lo[k];
      a.seg_nx[at] = s.nx[k];
      a.seg_row[at] = row;
      at++;
      row += s.hi[k] - s.lo[k] + 1;
    }
}

// rows [r0, r0 + nr) of the call (shard-local numbering) into out_id / out_nx [0, nr); nseg segments in the table
__global__ __launch_bounds__(JG_BLOCK) void k_read_rows(const uint64_t* __restrict__ seg_lo, const uint64_t* __restrict__ seg_nx,
                                                        const uint64_t* __restrict__ seg_row, uint64_t nseg, uint64_t r0,
                                                        uint64_t nr, uint64_t* __restrict__ out_id, uint64_t* __restrict__ out_nx) {
  // [thread][item] with one word of padding per thread: the stretch writes and the column reads spread over the banks
  __shared__ uint64_t l_id[JG_BLOCK * (JG_READ_ITEMS + 1)], l_nx[JG_BLOCK * (JG_READ_ITEMS + 1)];
  const uint64_t tile = (uint64_t)blockIdx.x * JG_READ_TILE;
  const uint64_t first = tile + (uint64_t)threadIdx.x * JG_READ_ITEMS;  // (piece-relative)
  if (first < nr) {
    const uint64_t r = r0 + first;
    uint64_t lo = 0, hi = nseg;  // the last segment with seg_row <= r: seg_row[lo] <= r < seg_row[hi]
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (seg_row[mid] <= r) lo = mid;
      else hi = mid;
    }
    uint64_t s = lo, s_first = seg_row[s], s_next = s + 1 < nseg ? seg_row[s + 1] : ~0ull;
    uint64_t s_lo = seg_lo[s], s_nx = seg_nx[s];
#pragma unroll
    for (uint32_t k = 0; k < JG_READ_ITEMS; k++) {
      const uint64_t q = r + k;
      if (first + k < nr) {
        if (q >= s_next) {  // (segments hold one row at least: one step per row at most)
          s++;
          s_first = s_next;
          s_next = s + 1 < nseg ? seg_row[s + 1] : ~0ull;
          s_lo = seg_lo[s], s_nx = seg_nx[s];
        }
        const uint64_t id = s_lo + (q - s_first);
        l_id[threadIdx.x * (JG_READ_ITEMS + 1) + k] = id;
        l_nx[threadIdx.x * (JG_READ_ITEMS + 1) + k] = q == s_first ? s_nx : id - 1;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < JG_READ_ITEMS; k++) {
    const uint32_t x = k * JG_BLOCK + threadIdx.x;  // tile-relative row: consecutive threads, consecutive rows
    const uint64_t q = tile + x;
    if (q < nr) {
      const uint32_t at = (x / JG_READ_ITEMS) * (JG_READ_ITEMS + 1) + x % JG_READ_ITEMS;
      out_id[q] = l_id[at];
      out_nx[q] = l_nx[at];
    }
  }
}
