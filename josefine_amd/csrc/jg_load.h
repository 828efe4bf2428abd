// jg_load.h — gfx950 kernels of jg_engine_load_chains: Chain::new (chain.rs:117-137) of a whole range of groups on the
// sled trees a process left behind (follower.rs:68-95), the trees given as CSR rows (one row per stored block, ids
// ascending within a group = sled's key order).  No thread and no wave walks a group: a group of 10^6 blocks is 10^6
// rows of the row passes like any other, and the per-group pass reads a bounded number of words per group.
//
//   k_load_flags     per row: its group (binary search in off), the ascending-order check (device error word, before
//                    anything is written), the segment-start flag; tile sums of the flags
//   k_scan_block_sums  (jg_sparse.h) the tile sums -> exclusive prefixes
//   k_load_scan      per row: the exclusive prefix of the start flags (= global segment index of a start row)
//   k_load_place     per row: a start row learns its rank within its group and writes lo / lo_next of window slot
//                    rank - (genesis present); the last row of a segment writes hi (the run's: run_hi)
//   k_load_groups    per group: flag word (NO_GENESIS, window count, commit key), the overflow / genesis-parent
//                    faults, then the JG_CMD_RESTART logic (jg_restart) and jg_store on the placed chain
#pragma once
#include "jg_device.h"
#include "jg_sparse.h"  // jg_block_exclusive_scan, JgScanJob, k_scan_block_sums

#define JG_LOAD_ITEMS 4u  // rows per thread in the flag / scan passes (a tile of 1024 rows: fewer tile sums to scan)
#define JG_LOAD_TILE (JG_BLOCK * JG_LOAD_ITEMS)

struct JgLoadArgs {
  uint32_t n;             // groups of the image (this shard's part)
  uint32_t g0;            // first group (shard-local numbering)
  uint64_t rows;          // off[n]
  const uint64_t* off;    // [n + 1], off[0] == 0
  const uint64_t* id;     // [rows]
  const uint64_t* next;   // [rows]
  const uint64_t* commit; // [n]
  const uint8_t* has_commit;  // [n]
  uint8_t* st;            // [rows] segment-start flags
  uint32_t* sx;           // [rows] exclusive prefix of st
  uint64_t* bsum;         // [tiles] tile sums, then their exclusive prefixes
  uint64_t* total;        // [1] number of segments of the image
  uint32_t* err;          // [1] 1: ids not strictly ascending within a group
};

// the group of row r: the last i with off[i] <= r (empty groups have off[i] == off[i + 1] and are skipped)
__device__ __forceinline__ uint32_t jg_load_group_of(const JgLoadArgs& a, uint64_t r) {
  uint32_t lo = 0, hi = a.n;  // off[lo] <= r < off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.off[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(JG_BLOCK) void k_load_flags(JgLoadArgs a) {
  const uint64_t base = (uint64_t)blockIdx.x * JG_LOAD_TILE + (uint64_t)threadIdx.x * JG_LOAD_ITEMS;
  uint32_t cnt = 0, bad = 0;
  if (base < a.rows) {
#pragma unroll
    for (uint32_t k = 0; k < JG_LOAD_ITEMS; k++) {
      const uint64_t r = base + k;
      if (r >= a.rows) break;
      const uint32_t i = jg_load_group_of(a, r);  // (a search per row: any number of empty groups may lie between two rows)
      const uint64_t id = a.id[r], nx = a.next[r];
      const bool first = r == a.off[i];
      const uint64_t prev = first ? 0 : a.id[r - 1];
      if (!first && id <= prev) bad = 1;
      const bool start = first || id != prev + 1 || nx != id - 1;
      a.st[r] = start ? 1 : 0;
      cnt += start ? 1u : 0u;
    }
  }
  if (__ballot(bad) && (threadIdx.x & 63u) == 0) atomicOr(a.err, 1u);
  uint32_t tot;
  (void)jg_block_exclusive_scan(cnt, &tot);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(JG_BLOCK) void k_load_scan(JgLoadArgs a) {
  if (*a.err) return;  // a refused image: nothing is written
  const uint64_t base = (uint64_t)blockIdx.x * JG_LOAD_TILE + (uint64_t)threadIdx.x * JG_LOAD_ITEMS;
  uint32_t f[JG_LOAD_ITEMS], v = 0;
#pragma unroll
  for (uint32_t k = 0; k < JG_LOAD_ITEMS; k++) {
    f[k] = base + k < a.rows ? a.st[base + k] : 0u;
    v += f[k];
  }
  uint32_t tot;
  uint32_t s = (uint32_t)a.bsum[blockIdx.x] + jg_block_exclusive_scan(v, &tot);
#pragma unroll
  for (uint32_t k = 0; k < JG_LOAD_ITEMS; k++) {
    if (base + k < a.rows) a.sx[base + k] = s;
    s += f[k];
  }
}

__global__ __launch_bounds__(JG_BLOCK) void k_load_place(JgDev d, JgLoadArgs a) {
  if (*a.err) return;
  const uint64_t r = (uint64_t)blockIdx.x * JG_BLOCK + threadIdx.x;
  if (r >= a.rows) return;
  const uint32_t i = jg_load_group_of(a, r);
  const uint64_t r0 = a.off[i], r1 = a.off[i + 1];
  const bool start = a.st[r] != 0;
  const bool end = r + 1 == r1 || a.st[r + 1] != 0;
  if (!start && !end) return;
  const uint32_t rank = a.sx[r] + (start ? 1u : 0u) - 1u - a.sx[r0];  // segment of row r within its group
  const uint32_t gen = a.id[r0] == 0 ? 1u : 0u;  // the group's first segment starts at genesis: it is the run
  const uint32_t g = a.g0 + i;
  if (gen && rank == 0) {
    if (end) d.run_hi[g] = a.id[r];
    return;
  }
  const uint32_t w = rank - gen;
  if (w >= JG_CHAIN_WINDOW) return;  // overflow: k_load_groups raises the fault
  const size_t at = (size_t)w * d.G + g;
  if (start) {
    d.win_lo[at] = a.id[r];
    d.win_next[at] = a.next[r];
  }
  if (end) d.win_hi[at] = a.id[r];
}

__global__ __launch_bounds__(JG_BLOCK) void k_load_groups(JgDev d, JgLoadArgs a, uint64_t now, uint32_t seq) {
  if (*a.err) return;
  const uint32_t i = blockIdx.x * JG_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t r0 = a.off[i], r1 = a.off[i + 1];
  const uint32_t nseg = r0 == r1 ? 0u : (uint32_t)((r1 == a.rows ? *a.total : a.sx[r1]) - a.sx[r0]);
  const bool gen = r0 != r1 && a.id[r0] == 0;
  JgLane L;
  jg_load(d, L, a.g0 + i);
  L.now = now;
  L.seq = seq;
  L.mp = L.mend = nullptr;
  L.fp = L.fend = nullptr;
  const uint32_t extra = nseg - (gen ? 1u : 0u);
  uint32_t f = 0;
  if (extra > JG_CHAIN_WINDOW) f = JG_FAULT_ENGINE_WINDOW_OVERFLOW;
  if (gen && a.next[r0] != 0) f = JG_FAULT_ENGINE_WINDOW_OVERFLOW;  // genesis' parent is implicit (jg_chain_insert)
  L.flags &= ~(JGF_WIN_MASK | JGF_NO_GENESIS | JGF_COMMIT_KEY | JGF_RUN | JGF_FAST);
  L.flags |= (extra > JG_CHAIN_WINDOW ? JG_CHAIN_WINDOW : extra) << JGF_WIN_SHIFT;
  if (gen) L.run_hi = d.run_hi[a.g0 + i];  // (k_load_place's)
  else L.flags |= JGF_NO_GENESIS;
  L.commit = 0;
  if (a.has_commit[i]) {
    L.flags |= JGF_COMMIT_KEY;
    L.commit = a.commit[i];
  }
  jg_restart(d, L);  // Raft::<Follower>::new + Chain::new (Q8) on the placed chain, the timer's next draw
  if (f) jg_raise(d, L, f);
  jg_store(d, L);
}
