// jg_compact.h — the pieces every feed's kernels share: the two passes of a stream compaction over 64-bit ballots, and the
// reduction of a workgroup's - then of all workgroups' - record of 8-byte words.  One copy each: jg_hosting.h, jg_watch.h,
// jg_isr.h, jg_isr_clock.h, jg_commits.h, jg_await.h and jg_poll.h keep their loads, views, rows and shadows and call these.
//
//   jg_tile_counts   pass 1's tail: wave-uniform counts through LDS, thread x gets the workgroup's total of count x
//   jg_rank_in_row   pass 2's middle: of one row the set bits before this lane's in the workgroup (ballot bits below + the
//                    waves before, through LDS: jg_wave_counts) and the row's total;  jg_rank_in_tile: a tile of one row
//   jg_ranked_rows   pass 2's skeleton over it: emit(k, pos) for the set bits whose pos < cap, pos ascending with the slot
//   jg_block_words   a wave's record of WORDS values through LDS, thread x folds column x into part[block][x]
//   jg_parts_reduce  one workgroup folds the partial records word by word: the body of the *_sum kernels
// A word folds as a sum, or as a maximum where is_max(x) says so (jg_fold).  The LDS arrays are the helpers' own
// (`__shared__` in a device function, as jg_block_exclusive_scan of jg_sparse.h): every helper but jg_parts_reduce is a
// barrier of the workgroup, and a kernel that calls one in a loop over tiles keeps a second barrier behind its use.
#pragma once
#include "jg_device.h"

#define JG_WAVES (JG_BLOCK / 64)

__device__ __forceinline__ uint32_t jg_clamp32(uint64_t x) { return x > 0xffffffffull ? 0xffffffffu : (uint32_t)x; }

__device__ __forceinline__ uint64_t jg_wave_sum64(uint64_t v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // (lane 0 holds the sum)
}
__device__ __forceinline__ uint64_t jg_wave_max64(uint64_t v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const uint64_t o = __shfl_down(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t jg_fold(uint64_t t, uint64_t p, bool is_max) { return is_max ? (p > t ? p : t) : t + p; }
struct JgNeverMax {  // is_max of a record that is sums only
  __device__ __forceinline__ bool operator()(uint32_t) const { return false; }
};

// c[x]: wave-uniform.  Thread x < N returns the workgroup's total of c[x] (any other thread 0)
template <uint32_t N>
__device__ __forceinline__ uint32_t jg_tile_counts(const uint32_t* c) {
  __shared__ uint32_t wave_n[N][JG_WAVES];
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (uint32_t x = 0; x < N; x++) wave_n[x][threadIdx.x >> 6] = c[x];
  }
  __syncthreads();
  uint32_t t = 0;
  if (threadIdx.x < N) {
#pragma unroll
    for (uint32_t w = 0; w < JG_WAVES; w++) t += wave_n[threadIdx.x][w];
  }
  return t;
}
__device__ __forceinline__ uint32_t jg_tile_count(uint32_t c) { return jg_tile_counts<1>(&c); }

// bit l of m[k]: lane l of this wave, row k.  The waves' popcounts through LDS: [k][w] = wave w's set bits of row k
typedef uint32_t JgWaveCounts[JG_WAVES];
template <uint32_t ROWS>
__device__ __forceinline__ const JgWaveCounts* jg_wave_counts(const uint64_t* m) {
  __shared__ JgWaveCounts wave_n[ROWS];
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (uint32_t k = 0; k < ROWS; k++) wave_n[k][threadIdx.x >> 6] = __popcll(m[k]);
  }
  __syncthreads();
  return wave_n;
}
// behind it, of one row: the set bits that belong to the lanes before this one in the workgroup; *row = the row's set bits
__device__ __forceinline__ uint32_t jg_rank_in_row(const JgWaveCounts& wave_n, uint64_t m, uint32_t* row) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t below = lane ? (~0ull >> (64u - lane)) : 0ull;  // the lanes below this one
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < JG_WAVES; w++) {
    before += w < wave ? wave_n[w] : 0u;
    all += wave_n[w];
  }
  *row = all;
  return before + __popcll(m & below);
}
__device__ __forceinline__ uint32_t jg_rank_in_tile(uint64_t m) {  // a tile of one row
  uint32_t row;
  return jg_rank_in_row(jg_wave_counts<1>(&m)[0], m, &row);
}

// the rows of a tile in order, `base` set bits before the tile: emit(k, pos) on the lane of every set bit of m[k] whose
// position pos among all set bits is below cap
template <uint32_t ROWS, class Emit>
__device__ __forceinline__ void jg_ranked_rows(const uint64_t* m, uint64_t base, uint64_t cap, Emit emit) {
  const JgWaveCounts* wave_n = jg_wave_counts<ROWS>(m);
#pragma unroll
  for (uint32_t k = 0; k < ROWS; k++) {
    uint32_t row;
    const uint64_t pos = base + jg_rank_in_row(wave_n[k], m[k], &row);
    if (((m[k] >> (threadIdx.x & 63u)) & 1ull) && pos < cap) emit(k, pos);
    base += row;
  }
}

// vals: this lane's record, each word already reduced over the wave into lane 0
template <uint32_t WORDS, class IsMax>
__device__ __forceinline__ void jg_block_words(const uint64_t* vals, IsMax is_max, uint64_t* part) {
  __shared__ uint64_t wave_b[JG_WAVES][WORDS];
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (uint32_t x = 0; x < WORDS; x++) wave_b[threadIdx.x >> 6][x] = vals[x];
  }
  __syncthreads();
  if (threadIdx.x < WORDS) {
    const bool mx = is_max(threadIdx.x);
    uint64_t t = 0;
#pragma unroll
    for (uint32_t w = 0; w < JG_WAVES; w++) t = jg_fold(t, wave_b[w][threadIdx.x], mx);
    part[(size_t)blockIdx.x * WORDS + threadIdx.x] = t;
  }
}

// one workgroup: wave w folds words w, w + 4, ... over the partial records, its lanes side by side over the records
template <uint32_t WORDS, class IsMax>
__device__ __forceinline__ void jg_parts_reduce(const uint64_t* part, uint32_t parts, uint64_t* out, IsMax is_max) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t x = threadIdx.x >> 6; x < WORDS; x += JG_WAVES) {  // (uniform over the wave)
    const bool mx = is_max(x);
    uint64_t t = 0;
    for (uint32_t b = lane; b < parts; b += 64) t = jg_fold(t, part[(size_t)b * WORDS + x], mx);
    t = mx ? jg_wave_max64(t) : jg_wave_sum64(t);
    if (lane == 0) out[x] = t;
  }
}
