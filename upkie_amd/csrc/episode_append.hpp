// episode_append.hpp -- the ordered append of a step's finished episodes, shared by episodes_step_kernel (episodes.hpp)
// and eval_step_kernel (eval_episodes.hpp): the grid, the head of the workspace, and the three device steps of the order.
//
// One launch per env step. Block b owns envs [b R, (b + 1) R) and walks them 256 at a time in env order. In each chunk
// an env that finishes its episode gets the next free index of the block's segment of the workspace, in env order (a
// wave ballot and a prefix over the block's four waves: episode_append_index), and the kernel stores its payload
// there; behind its chunks the block writes its count of finished episodes. Then the ticket (block_reduce.hpp): the
// block that arrives last does the ordered work alone. An exclusive prefix of the blocks' counts in LDS
// (episode_append_offsets) gives every finished episode of the step its index g in env order; episode g lies in the
// segment of the last block b with offsets[b] <= g (empty blocks share their offset with the next one), at
// b R + (g - offsets[b]), found by a binary search (episode_append_source). The last block reads one count per block:
// the same bits every call and under graph replay. The workspace: the ticket's 256 bytes, EPISODES_MAX_BLOCKS counts,
// then per payload field an array of num_envs entries (block b's finished episodes at [b R, b R + counts[b])).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace upkie {

enum { EPISODES_THREADS = 256, EPISODES_MAX_BLOCKS = 1024, EPISODES_COUNTS_OFFSET = 256 };
enum { EPISODES_SEGMENTS_OFFSET = EPISODES_COUNTS_OFFSET + EPISODES_MAX_BLOCKS * 4 };  // bytes ahead of the segments
// Grid for num_envs envs and its envs per block (every block owns at least one env).
inline int episodes_blocks(int num_envs, int* rows) {
  int g = (num_envs + EPISODES_THREADS - 1) / EPISODES_THREADS;
  g = g > EPISODES_MAX_BLOCKS ? EPISODES_MAX_BLOCKS : g;
  const int r = (num_envs + g - 1) / g;
  if (rows) *rows = r;
  return (num_envs + r - 1) / r;
}

// Grid of the reset kernels: one block per 256 envs under the step grid's cap (they stride over the rest).
inline int episodes_reset_blocks(int num_envs) {
  return num_envs > EPISODES_MAX_BLOCKS * EPISODES_THREADS ? EPISODES_MAX_BLOCKS : (num_envs + EPISODES_THREADS - 1) / EPISODES_THREADS;
}

// Bytes ahead of a payload field whose predecessors take `bytes_per_env`: its offset; with the whole payload's, the workspace's size.
inline int64_t episode_append_bytes(int num_envs, int bytes_per_env) { return EPISODES_SEGMENTS_OFFSET + (int64_t)num_envs * bytes_per_env; }
// The workspace carved: a payload field starts at segment(bytes per env of the fields before it); the segments start at segment(0).
struct EpisodeAppendWorkspace {
  unsigned* ticket;
  int32_t* counts;  // [EPISODES_MAX_BLOCKS]
  char* base;
  int num_envs;
  template <class T> T* segment(int bytes_before) const { return (T*)(base + episode_append_bytes(num_envs, bytes_before)); }
};
inline EpisodeAppendWorkspace episode_append_carve(void* workspace, int num_envs) {
  char* ws = (char*)workspace;
  return {(unsigned*)ws, (int32_t*)(ws + EPISODES_COUNTS_OFFSET), ws, num_envs};
}

#if defined(__HIPCC__)
// One chunk of 256 envs, every thread of the block: the index inside the block's segment of this thread's finished episode
// (meaningful where `done`), `done_in_block` moved on by the chunk's count. Two barriers; wave_n: LDS, one word per wave.
__device__ __forceinline__ int episode_append_index(bool done, int& done_in_block, int32_t* wave_n) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long ballot = __ballot(done);
  const int before = __popcll(ballot & ((1ull << lane) - 1ull));
  if (lane == 0) wave_n[wave] = __popcll(ballot);
  __syncthreads();
  int at = done_in_block + before;
  for (int w = 0; w < wave; ++w) at += wave_n[w];
  for (int w = 0; w < EPISODES_THREADS / 64; ++w) done_in_block += wave_n[w];
  __syncthreads();
  return at;
}

// The last block: offsets[b] = counts[0] + ... + counts[b - 1] for b = 0 .. EPISODES_MAX_BLOCKS, four counts per thread and an
// inclusive scan of the threads' sums (Hillis-Steele) between them. Returns the step's total. LDS: scan [256], offsets [1025].
__device__ __forceinline__ int episode_append_offsets(const int32_t* counts, int blocks, int32_t* scan, int32_t* offsets) {
  constexpr int PER = EPISODES_MAX_BLOCKS / EPISODES_THREADS;  // blocks per thread
  const int tid = threadIdx.x;
  int own[PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int b = tid * PER + k;
    own[k] = b < blocks ? counts[b] : 0;
    sum += own[k];
  }
  scan[tid] = sum;
  __syncthreads();
  for (int d = 1; d < EPISODES_THREADS; d <<= 1) {
    const int add = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  int run = scan[tid] - sum;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    offsets[tid * PER + k] = run;
    run += own[k];
  }
  if (tid == EPISODES_THREADS - 1) offsets[EPISODES_MAX_BLOCKS] = run;
  __syncthreads();
  return offsets[EPISODES_MAX_BLOCKS];
}

// Where finished episode g lies in a segment array: b rows + (g - offsets[b]), b the last block with offsets[b] <= g.
__device__ __forceinline__ int episode_append_source(int g, const int32_t* offsets, int blocks, int rows) {
  int lo = 0, hi = blocks - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= g) lo = mid;
    else hi = mid - 1;
  }
  return lo * rows + (g - offsets[lo]);
}

#endif  // __HIPCC__

}  // namespace upkie
