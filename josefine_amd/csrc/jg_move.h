// jg_move.h — gfx950 kernels of jg_engine_export_groups / jg_engine_import_groups: a group's whole state moved between the
// SoA columns of jg_device.h and one fixed-stride record per group (the state image), raw - not re-derived: the lag-packed
// mlag, the escape slots of match_wide and the stale id_gen / run_hi columns of RUN / FAST chains travel as they are.
// Both directions are a transpose through LDS, a tile of JG_MOVE_TILE groups per workgroup:
//
//   k_export_groups  every column row of the tile (the [R][G] and [W][G] columns row by row, the two uint4 cold arrays as
//                    16-byte loads) -> the tile in record layout in LDS; the check words; the tile leaves as contiguous
//                    16-byte stores of whole records
//   k_import_check   the records in (16-byte loads) -> LDS; check words and field ranges -> the error word, the own slots
//                    seen -> a mask (the host's uniform_self)
//   k_import_groups  the inverse transpose, plus the time shift and the irregular_seen rule; returns at once when the
//                    error word is set, so a refused image writes nothing
//
// Record layout (8-byte words; DESIGN.md "Handing groups over"): word 0 the check word, then term, commit, head, id_gen,
// run_hi, mlag, heartbeat_time, flags (low half; the high half 0), cold_t (2 words), cold_v (2), fvote_id (4 words, two ids
// each), win_lo[W], win_hi[W], win_next[W], match_wide[R], zeros up to the stride.  The stride is a multiple of 64 B:
// 384 B for R <= 7, 448 B for R = 8.
#pragma once
#include "jg_device.h"

#define JG_MOVE_TILE 64u  // groups per workgroup: one wave's row of a column
#define JG_MOVE_W_TERM 1u
#define JG_MOVE_W_FLAGS 8u
#define JG_MOVE_W_COLD 9u
#define JG_MOVE_W_FVOTE 13u
#define JG_MOVE_W_WIN (JG_MOVE_W_FVOTE + JG_FOREIGN_VOTERS / 2u)  // win_lo, then win_hi, then win_next
#define JG_MOVE_W_MATCH (JG_MOVE_W_WIN + 3u * JG_CHAIN_WINDOW)   // 41
#define JG_MOVE_ROWS_FIXED (JG_MOVE_W_MATCH + 1u)                // column rows of a tile besides match_wide: 42
#define JG_MOVE_KEY 0x6a6f73656d6f7665ull                         // seeds the check word
// (the layout and the passes below are written for these: four lanes fold one record's check word, a 256-lane workgroup a
// tile of 64 records; two foreign voter ids share a word)
static_assert(JG_BLOCK == 4 * JG_MOVE_TILE, "jg_move_check: four lanes per record of a tile");
static_assert(JG_FOREIGN_VOTERS == 8, "the record holds fvote_id[8] in words 13-16");
static_assert(JG_CHAIN_WINDOW == 8 && JG_MAX_REPLICAS == 8, "the record layout of DESIGN.md \"Handing groups over\"");

// words per record (a multiple of 8: a 64-byte stride) for R replicas
__host__ __device__ __forceinline__ uint32_t jg_move_words(uint32_t R) { return (JG_MOVE_W_MATCH + R + 7u) & ~7u; }

// the check word of a record: every word but word 0 hashed with its index, XOR-folded (a bijection per word: a change
// of any one word always changes the fold).  Word k's term:
__device__ __forceinline__ uint64_t jg_move_term(uint64_t w, uint32_t k) { return jg_mix64(w ^ (uint64_t)k * 0x9e3779b97f4a7c15ull); }

struct JgMoveArgs {
  uint32_t g0, n;       // shard-local groups [g0, g0 + n)
  uint64_t shift;       // import: added (mod 2^64) to election_time and heartbeat_time
  uint4* out;           // export: [n] records
  const uint4* in;      // import: [n] records
  uint32_t* err;        // import: [2] {bit 0: a record failed its check or a range, bit 1: per-step state of a destination
                        // group is not empty (internal); own slots seen (bit s)}
};

// LDS image of a tile: record i's 32-bit word q at s[i * P + q], P = 2 * NW + 1 (odd: the 64 lanes writing one column
// row for 64 records hit 64 different banks)
template <uint32_t NW>
struct JgMoveTileLds {
  static constexpr uint32_t P = 2 * NW + 1;
  uint32_t s[JG_MOVE_TILE * P];
};

// column row `row` of the tile's record i (group g): read it from the columns into LDS (export) or back (import)
template <uint32_t NW, bool EXPORT>
__device__ __forceinline__ void jg_move_row(const JgDev& d, uint32_t* s, uint32_t row, uint32_t i, uint32_t g, uint64_t shift) {
  uint32_t* w = s + i * JgMoveTileLds<NW>::P;
  const size_t G = d.G;
  uint64_t* col = nullptr;  // an 8-byte column: the word at record word `k`
  uint32_t k = 0;
  if (row < 7u) {  // (a branch per column, not an array of pointers: that would live in scratch)
    col = row == 0 ? d.term : row == 1 ? d.commit : row == 2 ? d.head : row == 3 ? d.id_gen : row == 4 ? d.run_hi : row == 5 ? d.mlag : d.heartbeat_time;
    col += g, k = JG_MOVE_W_TERM + row;
  } else if (row == 7u) {  // flags
    if (EXPORT) w[2 * JG_MOVE_W_FLAGS] = d.flags[g], w[2 * JG_MOVE_W_FLAGS + 1] = 0u;
    else d.flags[g] = w[2 * JG_MOVE_W_FLAGS];
    return;
  } else if (row < 10u) {  // the two cold arrays, 16 bytes each
    uint4* c = (row == 8u ? d.cold.t : d.cold.v) + g;
    uint32_t* q = w + 2 * (JG_MOVE_W_COLD + 2u * (row - 8u));
    if (EXPORT) {
      const uint4 v = *c;
      q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
    } else {
      uint64_t t = (uint64_t)q[0] | (uint64_t)q[1] << 32;
      if (row == 8u) t += shift;  // election_time
      *c = make_uint4((uint32_t)t, (uint32_t)(t >> 32), q[2], q[3]);
    }
    return;
  } else if (row < 10u + JG_FOREIGN_VOTERS) {  // fvote_id, 4 bytes
    uint32_t* c = d.fvote_id + (size_t)(row - 10u) * G + g;
    uint32_t* q = w + 2 * JG_MOVE_W_FVOTE + (row - 10u);
    if (EXPORT) *q = *c;
    else *c = *q;
    return;
  } else if (row < 10u + JG_FOREIGN_VOTERS + 3u * JG_CHAIN_WINDOW) {  // win_lo, win_hi, win_next
    const uint32_t r = row - 10u - JG_FOREIGN_VOTERS, a = r / JG_CHAIN_WINDOW, x = r % JG_CHAIN_WINDOW;
    col = (a == 0 ? d.win_lo : a == 1 ? d.win_hi : d.win_next) + (size_t)x * G + g, k = JG_MOVE_W_WIN + r;
  } else {  // match_wide
    const uint32_t r = row - JG_MOVE_ROWS_FIXED;
    col = d.match_wide + (size_t)r * G + g, k = JG_MOVE_W_MATCH + r;
  }
  if (EXPORT) {
    const uint64_t v = *col;
    w[2 * k] = (uint32_t)v, w[2 * k + 1] = (uint32_t)(v >> 32);
  } else {
    uint64_t v = (uint64_t)w[2 * k] | (uint64_t)w[2 * k + 1] << 32;
    if (k == JG_MOVE_W_TERM + 6u) v += shift;  // heartbeat_time
    *col = v;
  }
}

// the check word of record i of the tile (4 lanes per record, lanes 4i .. 4i + 3 of the workgroup; all 256 lanes call it)
template <uint32_t NW>
__device__ __forceinline__ uint64_t jg_move_check(const uint32_t* s) {
  const uint32_t i = threadIdx.x >> 2, part = threadIdx.x & 3u;
  const uint32_t* w = s + i * JgMoveTileLds<NW>::P;
  uint64_t c = part == 0 ? jg_mix64(JG_MOVE_KEY ^ NW) : 0ull;
  for (uint32_t k = 1 + part; k < NW; k += 4) c ^= jg_move_term((uint64_t)w[2 * k] | (uint64_t)w[2 * k + 1] << 32, k);
  uint32_t lo = (uint32_t)c, hi = (uint32_t)(c >> 32);
  lo ^= __shfl_xor(lo, 1, 64), hi ^= __shfl_xor(hi, 1, 64);
  lo ^= __shfl_xor(lo, 2, 64), hi ^= __shfl_xor(hi, 2, 64);
  return (uint64_t)lo | (uint64_t)hi << 32;
}

// records [t0, t0 + nt) of the call between global memory and the tile in LDS, as 16-byte pieces (NW / 2 per record)
template <uint32_t NW>
__device__ __forceinline__ void jg_move_tile_in(uint32_t* s, const uint4* in, uint32_t nt) {
  constexpr uint32_t C = NW / 2, P = JgMoveTileLds<NW>::P;
  for (uint32_t c = threadIdx.x; c < nt * C; c += JG_BLOCK) {
    const uint4 v = in[c];
    uint32_t* q = s + (c / C) * P + (c % C) * 4;
    q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
  }
}

template <uint32_t NW>
__global__ __launch_bounds__(JG_BLOCK) void k_export_groups(JgDev d, JgMoveArgs a) {
  __shared__ JgMoveTileLds<NW> t;
  constexpr uint32_t P = JgMoveTileLds<NW>::P, C = NW / 2;
  const uint32_t t0 = blockIdx.x * JG_MOVE_TILE, nt = min(JG_MOVE_TILE, a.n - t0);
  const uint32_t rows = JG_MOVE_ROWS_FIXED + d.R;
  // column rows: a wave takes one row of one column for the tile's 64 groups (contiguous lanes)
  for (uint32_t k = threadIdx.x; k < rows * JG_MOVE_TILE; k += JG_BLOCK) {
    const uint32_t row = k / JG_MOVE_TILE, i = k % JG_MOVE_TILE;
    if (i < nt) jg_move_row<NW, true>(d, t.s, row, i, a.g0 + t0 + i, 0);
  }
  for (uint32_t k = threadIdx.x; k < (NW - JG_MOVE_W_MATCH - d.R) * JG_MOVE_TILE; k += JG_BLOCK) {  // the padding: zeros
    const uint32_t i = k % JG_MOVE_TILE, q = 2 * (JG_MOVE_W_MATCH + d.R + k / JG_MOVE_TILE);
    t.s[i * P + q] = 0u, t.s[i * P + q + 1] = 0u;
  }
  __syncthreads();
  const uint64_t c = jg_move_check<NW>(t.s);
  if ((threadIdx.x & 3u) == 0) {
    uint32_t* w = t.s + (threadIdx.x >> 2) * P;
    w[0] = (uint32_t)c, w[1] = (uint32_t)(c >> 32);
  }
  __syncthreads();
  uint4* out = a.out + (size_t)t0 * C;
  for (uint32_t k = threadIdx.x; k < nt * C; k += JG_BLOCK) {
    const uint32_t* q = t.s + (k / C) * P + (k % C) * 4;
    out[k] = make_uint4(q[0], q[1], q[2], q[3]);
  }
}

// Per-step transient state is empty between calls: a dense kernel's deferral bits are consumed and cleared by the slow
// kernel behind it in the same step (k_dense_slow, k_follower_slow; the slow lists' counts likewise), so nothing of the
// destination's groups is left to be picked up by a later pass.  Asserted here for the groups about to be written.
__device__ __forceinline__ bool jg_move_deferred(const JgDev& d, uint32_t g) {
  const uint32_t w = g >> 6, words = (d.G + 63u) >> 6;
  const uint64_t bit = 1ull << (g & 63u);
  return ((d.defer_bits[w] | d.fdefer_bits[w] | d.fdefer_bits[words + w]) & bit) != 0;
}

template <uint32_t NW>
__global__ __launch_bounds__(JG_BLOCK) void k_import_check(JgDev d, JgMoveArgs a) {
  const uint32_t R = d.R;
  __shared__ JgMoveTileLds<NW> t;
  __shared__ uint32_t s_err, s_slots;
  constexpr uint32_t P = JgMoveTileLds<NW>::P, C = NW / 2;
  const uint32_t t0 = blockIdx.x * JG_MOVE_TILE, nt = min(JG_MOVE_TILE, a.n - t0);
  if (threadIdx.x == 0) s_err = 0u, s_slots = 0u;
  jg_move_tile_in<NW>(t.s, a.in + (size_t)t0 * C, nt);
  __syncthreads();
  const uint64_t c = jg_move_check<NW>(t.s);
  const uint32_t i = threadIdx.x >> 2;
  if ((threadIdx.x & 3u) == 0 && i < nt) {
    const uint32_t* w = t.s + i * P;
    const uint32_t f = w[2 * JG_MOVE_W_FLAGS];
    bool bad = c != ((uint64_t)w[0] | (uint64_t)w[1] << 32);
    bad |= (f & JGF_ROLE_MASK) > JG_ROLE_LEADER;
    bad |= ((f & JGF_SELF_MASK) >> JGF_SELF_SHIFT) >= R;
    bad |= ((f & JGF_WIN_MASK) >> JGF_WIN_SHIFT) > JG_CHAIN_WINDOW;
    bad |= w[2 * JG_MOVE_W_FLAGS + 1] != 0u;
    if (bad) atomicOr(&s_err, 1u);
    if (jg_move_deferred(d, a.g0 + t0 + i)) atomicOr(&s_err, 2u);
    atomicOr(&s_slots, 1u << ((f & JGF_SELF_MASK) >> JGF_SELF_SHIFT));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_err) atomicOr(a.err, s_err);
    atomicOr(a.err + 1, s_slots);
  }
}

template <uint32_t NW>
__global__ __launch_bounds__(JG_BLOCK) void k_import_groups(JgDev d, JgMoveArgs a) {
  if (*(volatile uint32_t*)a.err) return;  // a refused image: nothing is written
  __shared__ JgMoveTileLds<NW> t;
  constexpr uint32_t P = JgMoveTileLds<NW>::P, C = NW / 2;
  const uint32_t t0 = blockIdx.x * JG_MOVE_TILE, nt = min(JG_MOVE_TILE, a.n - t0);
  jg_move_tile_in<NW>(t.s, a.in + (size_t)t0 * C, nt);
  __syncthreads();
  const uint32_t rows = JG_MOVE_ROWS_FIXED + d.R;
  for (uint32_t k = threadIdx.x; k < rows * JG_MOVE_TILE; k += JG_BLOCK) {
    const uint32_t row = k / JG_MOVE_TILE, i = k % JG_MOVE_TILE;
    if (i < nt) jg_move_row<NW, false>(d, t.s, row, i, a.g0 + t0 + i, a.shift);
  }
  // jg_store's rule: a leader stored with a chain that is not in FAST form has the slow kernel scheduled behind the dense one
  if (threadIdx.x < nt) {
    const uint32_t f = t.s[threadIdx.x * P + 2 * JG_MOVE_W_FLAGS];
    if ((f & JGF_ROLE_MASK) == JG_ROLE_LEADER && !(f & JGF_FAST) && !(f & JGF_FAULT_MASK)) *d.irregular_seen = 1;
  }
}
