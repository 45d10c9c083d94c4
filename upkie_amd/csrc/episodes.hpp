// episodes.hpp -- Stable-Baselines3's Monitor + ep_info_buffer for a batch of envs, on the device: per env the running
// return (fp64) and length (int32) of its episode; a ring of the last `window` finished episodes (fp64 return, int32
// length) with its head and fill count; the count of all episodes; the mean return and mean length over the ring
// (include/upkie_hip.h states the arithmetic; Python: upkie_amd/episodes.py).
//
// One launch per env step. Block b owns envs [b R, (b + 1) R) and walks them 256 at a time in env order: every env adds
// (double)reward and 1 to its accumulators; an env with terminated | truncated set finishes its episode, zeroes its
// accumulators and appends (return, length) to the block's segment of the workspace, in env order (a wave ballot and
// a prefix over the block's four waves), and the block writes its count of finished episodes. Then the ticket
// (block_reduce.hpp): the block that arrives last does the ordered work alone: an
// exclusive prefix of the blocks' counts (in LDS) gives every finished episode of the step its index g in env order;
// of the `total` finished, the last keep = min(total, window) enter the ring at head, head + 1, ... (a deque of
// maxlen window: what more than `window` finishers push out of it never lands), each found by a binary search of the
// prefix; the means are recomputed in ring order, oldest to newest (the ring staged through LDS by the whole block, 1024
// entries at a time, then summed by one thread: the return sum sequential in fp64, the length sum exact in int64). The
// last block reads one count per block and at most `window` finished episodes: the same bits every call and under
// graph replay.
//
// Launch R (reset): the accumulators of the masked envs (all without a mask) back to zero; no episode is recorded and
// the ring is kept (Monitor.reset).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "block_reduce.hpp"

namespace upkie {

enum { EPISODES_THREADS = 256, EPISODES_MAX_BLOCKS = 1024, EPISODES_MAX_WINDOW = 65536, EPISODES_COUNTS_OFFSET = 256, EPISODES_STAGE = 1024 };

struct EpisodesDev {
  int num_envs, window;
  int rows, blocks;  // envs per block, the grid
  const float* reward;
  const uint8_t* terminated;
  const uint8_t* truncated;
  double* ep_return;    // [num_envs]
  int32_t* ep_length;   // [num_envs]
  double* ring_return;  // [window]
  int32_t* ring_length; // [window]
  int64_t* counters;    // total episodes, head, fill
  double* means;        // mean return, mean length over the ring
  unsigned* ticket;
  int32_t* counts;      // [blocks] finished episodes per block in this step
  double* fin_return;   // [num_envs]: block b's finished returns at [b rows, b rows + counts[b])
  int32_t* fin_length;  // [num_envs]
};

// Grid for num_envs envs and its envs per block (every block owns at least one env).
inline int episodes_blocks(int num_envs, int* rows) {
  int g = (num_envs + EPISODES_THREADS - 1) / EPISODES_THREADS;
  g = g > EPISODES_MAX_BLOCKS ? EPISODES_MAX_BLOCKS : g;
  const int r = (num_envs + g - 1) / g;
  if (rows) *rows = r;
  return (num_envs + r - 1) / r;
}

// Workspace bytes: the ticket, the per-block counts, then the finished returns and lengths.
inline int64_t episodes_workspace_bytes(int num_envs) {
  const int64_t counts = (int64_t)EPISODES_MAX_BLOCKS * 4;
  return EPISODES_COUNTS_OFFSET + counts + (int64_t)num_envs * 8 + (int64_t)num_envs * 4;
}

#if defined(__HIPCC__)

__global__ __launch_bounds__(EPISODES_THREADS) void episodes_step_kernel(const EpisodesDev P) {
  __shared__ int32_t offsets[EPISODES_MAX_BLOCKS + 1];  // last block: exclusive prefix of the counts, then the total
  __shared__ int32_t wave_n[EPISODES_THREADS / 64 + 1];  // finished per wave of a chunk; [4]: "last block" flag
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = blockIdx.x * P.rows, r1 = min(P.num_envs, r0 + P.rows);

  // every env: its accumulators; the finished ones appended to the block's segment in env order
  int done_in_block = 0;
  for (int c = r0; c < r1; c += EPISODES_THREADS) {
    const int i = c + tid;
    const bool valid = i < r1;
    bool done = false;
    double ret = 0.0;
    int len = 0;
    if (valid) {
      ret = P.ep_return[i] + (double)P.reward[i];
      len = P.ep_length[i] + 1;
      done = (P.terminated && P.terminated[i] != 0) || (P.truncated && P.truncated[i] != 0);
      P.ep_return[i] = done ? 0.0 : ret;
      P.ep_length[i] = done ? 0 : len;
    }
    const unsigned long long ballot = __ballot(done);
    const int before = __popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) wave_n[wave] = __popcll(ballot);
    __syncthreads();
    int base = done_in_block;
    for (int w = 0; w < wave; ++w) base += wave_n[w];
    if (done) {
      const int at = r0 + base + before;
      P.fin_return[at] = ret;
      P.fin_length[at] = len;
    }
    for (int w = 0; w < EPISODES_THREADS / 64; ++w) done_in_block += wave_n[w];
    __syncthreads();
  }
  if (tid == 0) P.counts[blockIdx.x] = done_in_block;

  // publish and draw a ticket (block_reduce.hpp); the last arriver goes on, with every block's count and segment visible
  if (!ticket_last_block(P.ticket, P.blocks, &wave_n[EPISODES_THREADS / 64])) return;
  constexpr int PER = EPISODES_MAX_BLOCKS / EPISODES_THREADS;  // blocks per thread in the prefix
  int own[PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int b = tid * PER + k;
    own[k] = b < P.blocks ? P.counts[b] : 0;
    sum += own[k];
  }
  // inclusive scan of the threads' sums (Hillis-Steele in LDS), then each thread's blocks
  __shared__ int32_t scan[EPISODES_THREADS];
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

  const int total = offsets[EPISODES_MAX_BLOCKS];
  const int window = P.window;
  const int keep = total < window ? total : window;
  const int first = total - keep;
  const int head = (int)P.counters[1], fill = (int)P.counters[2];
  for (int j = tid; j < keep; j += EPISODES_THREADS) {
    const int g = first + j;
    int lo = 0, hi = P.blocks - 1;  // the block b with offsets[b] <= g < offsets[b + 1] (the last such: empty blocks share offsets)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (offsets[mid] <= g) lo = mid;
      else hi = mid - 1;
    }
    const int src = lo * P.rows + (g - offsets[lo]);
    const int slot = head + j < window ? head + j : head + j - window;  // (head < window, j < keep <= window)
    P.ring_return[slot] = P.fin_return[src];
    P.ring_length[slot] = P.fin_length[src];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // the means over the ring, oldest to newest: the block stages EPISODES_STAGE entries at a time in LDS (loads in
  // parallel), then one thread sums them in order -- the return sum sequential in fp64, the length sum exact
  __shared__ double stage_r[EPISODES_STAGE];
  __shared__ int32_t stage_l[EPISODES_STAGE];
  const int new_fill = fill + keep < window ? fill + keep : window;
  const int new_head = head + keep < window ? head + keep : head + keep - window;
  const int oldest = new_head - new_fill < 0 ? new_head - new_fill + window : new_head - new_fill;
  double rs = 0.0;
  int64_t ls = 0;
  for (int k0 = 0; k0 < new_fill; k0 += EPISODES_STAGE) {
    const int cnt = min((int)EPISODES_STAGE, new_fill - k0);
    for (int k = tid; k < cnt; k += EPISODES_THREADS) {
      const int s = oldest + k0 + k < window ? oldest + k0 + k : oldest + k0 + k - window;  // (oldest < window, k0 + k < window)
      stage_r[k] = P.ring_return[s];
      stage_l[k] = P.ring_length[s];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll 8
      for (int k = 0; k < cnt; ++k) {
        rs += stage_r[k];
        ls += stage_l[k];
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    P.counters[0] += total;
    P.counters[1] = new_head;
    P.counters[2] = new_fill;
    P.means[0] = new_fill ? rs / (double)new_fill : 0.0;
    P.means[1] = new_fill ? (double)ls / (double)new_fill : 0.0;
  }
}

__global__ __launch_bounds__(EPISODES_THREADS) void episodes_reset_kernel(int num_envs, const uint8_t* __restrict__ mask, double* ep_return,
                                                                        int32_t* ep_length) {
  for (int i = blockIdx.x * EPISODES_THREADS + threadIdx.x; i < num_envs; i += gridDim.x * EPISODES_THREADS) {
    if (!mask || mask[i] != 0) {
      ep_return[i] = 0.0;
      ep_length[i] = 0;
    }
  }
}

#endif  // __HIPCC__

}  // namespace upkie
