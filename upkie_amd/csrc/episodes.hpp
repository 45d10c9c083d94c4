// episodes.hpp -- Stable-Baselines3's Monitor + ep_info_buffer for a batch of envs, on the device: per env the running
// return (fp64) and length (int32) of its episode; a ring of the last `window` finished episodes (fp64 return, int32
// length) with its head and fill count; the count of all episodes; the mean return and mean length over the ring
// (include/upkie_hip.h states the arithmetic; Python: upkie_amd/episodes.py).
//
// One launch per env step, the ordered append of episode_append.hpp. Every env counts: it adds (double)reward and 1 to
// its accumulators, and with terminated | truncated set it finishes its episode and zeroes them. The payload: (return,
// length). The last block keeps a ring: of the `total` finished, the last keep = min(total, window) enter it at head,
// head + 1, ... (a deque of maxlen window: what more than `window` finishers push out of it never lands); then the means
// are recomputed in ring order, oldest to newest (the ring staged through LDS by the whole block, 1024 entries at a time,
// then summed by one thread: the return sum sequential in fp64, the length sum exact in int64). It reads at most
// `window` finished episodes.
//
// Launch R (reset): the accumulators of the masked envs (all without a mask) back to zero; no episode is recorded and
// the ring is kept (Monitor.reset).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "block_reduce.hpp"
#include "episode_append.hpp"

namespace upkie {

enum { EPISODES_MAX_WINDOW = 65536, EPISODES_STAGE = 1024 };

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

// Workspace bytes: the head of episode_append.hpp, then the finished returns and lengths.
inline int64_t episodes_workspace_bytes(int num_envs) { return episode_append_bytes(num_envs, 8 + 4); }

#if defined(__HIPCC__)

__global__ __launch_bounds__(EPISODES_THREADS) void episodes_step_kernel(const EpisodesDev P) {
  __shared__ int32_t offsets[EPISODES_MAX_BLOCKS + 1];  // last block: exclusive prefix of the counts, then the total
  __shared__ int32_t wave_n[EPISODES_THREADS / 64 + 1];  // finished per wave of a chunk; [4]: "last block" flag
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * P.rows, r1 = min(P.num_envs, r0 + P.rows);

  // every env: its accumulators; the finished ones appended to the block's segment in env order
  int done_in_block = 0;
  for (int c = r0; c < r1; c += EPISODES_THREADS) {
    const int i = c + tid;
    bool done = false;
    double ret = 0.0;
    int len = 0;
    if (i < r1) {
      ret = P.ep_return[i] + (double)P.reward[i];
      len = P.ep_length[i] + 1;
      done = (P.terminated && P.terminated[i] != 0) || (P.truncated && P.truncated[i] != 0);
      P.ep_return[i] = done ? 0.0 : ret;
      P.ep_length[i] = done ? 0 : len;
    }
    const int at = r0 + episode_append_index(done, done_in_block, wave_n);
    if (done) {
      P.fin_return[at] = ret;
      P.fin_length[at] = len;
    }
  }
  if (tid == 0) P.counts[blockIdx.x] = done_in_block;

  // publish and draw a ticket (block_reduce.hpp); the last arriver goes on, with every block's count and segment visible
  if (!ticket_last_block(P.ticket, P.blocks, &wave_n[EPISODES_THREADS / 64])) return;
  __shared__ int32_t scan[EPISODES_THREADS];
  const int total = episode_append_offsets(P.counts, P.blocks, scan, offsets);
  const int window = P.window;
  const int keep = total < window ? total : window;
  const int first = total - keep;
  const int head = (int)P.counters[1], fill = (int)P.counters[2];
  for (int j = tid; j < keep; j += EPISODES_THREADS) {
    const int g = first + j;
    const int src = episode_append_source(g, offsets, P.blocks, P.rows);
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
