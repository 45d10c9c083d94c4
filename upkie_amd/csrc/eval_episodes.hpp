// eval_episodes.hpp -- the bookkeeping of Stable-Baselines3's evaluate_policy for a batch of envs, on the device: per env
// the running return (fp64) and length (int32) of its episode, the count of episodes it has given and its quota
// target[i] = (E + i) / N of the E = n_eval_episodes asked for; a list of E records (fp64 return, int32 length, env,
// whether the time limit ended it) with its fill count; once the list is full, its summary (include/upkie_hip.h states
// the arithmetic; Python: upkie_amd/evaluation.py).
//
// One launch per env step, the ordered append of episode_append.hpp. Only an env below its quota counts: it adds
// (double)reward and 1 to its accumulators, and with terminated | truncated set it finishes its episode, counts it and
// zeroes them; an env at its quota is neither read further nor written. The payload: (return, length, env,
// truncated & !terminated). The last block keeps a list: episode g becomes record filled + g (the quotas sum to E, so
// filled + g < E; the store is bounded by E all the same): records are step-major and env-minor, the order SB3's loop
// appends in. In the step in which filled reaches E it goes on to the summary: the records staged through LDS by the
// whole block, 1024 at a time, and added by one thread in record order -- the return sum sequential in fp64, the length
// sum exact in int64, the smallest and largest return, the count of time-limit records; then a second pass in the same
// order for sum((x - mean)^2) of the returns and of the lengths, each term rounded (no fused multiply-add). It reads at
// most E records.
//
// Launch R (reset): accumulators, counts, filled, steps and the summary back to zero, the targets written for E.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "block_reduce.hpp"
#include "episode_append.hpp"

namespace upkie {

enum { EVAL_STAGE = 1024, EVAL_SUMMARY_WORDS = 7 };

struct EvalDev {
  int num_envs, episodes;  // N, E
  int rows, blocks;        // envs per block, the grid
  const float* reward;
  const uint8_t* terminated;
  const uint8_t* truncated;
  double* ep_return;       // [num_envs]
  int32_t* ep_length;      // [num_envs]
  int32_t* count;          // [num_envs] episodes the env has given
  const int32_t* target;   // [num_envs] its quota
  double* rec_return;      // [episodes]
  int32_t* rec_length;     // [episodes]
  int32_t* rec_env;        // [episodes]
  uint8_t* rec_truncated;  // [episodes]
  int64_t* counters;       // filled, steps
  double* summary;         // [EVAL_SUMMARY_WORDS]
  unsigned* ticket;
  int32_t* counts;         // [blocks] finished episodes per block in this step
  double* fin_return;      // [num_envs]: block b's finished episodes at [b rows, b rows + counts[b])
  int32_t* fin_length;     // [num_envs]
  int32_t* fin_env;        // [num_envs]
  uint8_t* fin_truncated;  // [num_envs]
};

// Workspace bytes: the head of episode_append.hpp, then the finished returns, lengths, envs and time-limit flags.
inline int64_t eval_workspace_bytes(int num_envs) { return episode_append_bytes(num_envs, 8 + 4 + 4 + 1); }

#if defined(__HIPCC__)

__global__ __launch_bounds__(EPISODES_THREADS) void eval_step_kernel(const EvalDev P) {
  __shared__ int32_t offsets[EPISODES_MAX_BLOCKS + 1];  // last block: exclusive prefix of the counts, then the total
  __shared__ int32_t wave_n[EPISODES_THREADS / 64 + 1];  // finished per wave of a chunk; [4]: "last block" flag
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * P.rows, r1 = min(P.num_envs, r0 + P.rows);

  // every env below its quota: its accumulators; the finished ones appended to the block's segment in env order
  int done_in_block = 0;
  for (int c = r0; c < r1; c += EPISODES_THREADS) {
    const int i = c + tid;
    bool done = false, limit = false;
    double ret = 0.0;
    int len = 0;
    if (i < r1) {
      const int given = P.count[i];
      if (given < P.target[i]) {
        ret = P.ep_return[i] + (double)P.reward[i];
        len = P.ep_length[i] + 1;
        const bool term = P.terminated && P.terminated[i] != 0, trunc = P.truncated && P.truncated[i] != 0;
        done = term || trunc;
        limit = trunc && !term;
        P.ep_return[i] = done ? 0.0 : ret;
        P.ep_length[i] = done ? 0 : len;
        if (done) P.count[i] = given + 1;
      }
    }
    const int at = r0 + episode_append_index(done, done_in_block, wave_n);  // (< r1: at most one per env of the block)
    if (done) {
      P.fin_return[at] = ret;
      P.fin_length[at] = len;
      P.fin_env[at] = i;
      P.fin_truncated[at] = limit ? 1 : 0;
    }
  }
  if (tid == 0) P.counts[blockIdx.x] = done_in_block;

  // publish and draw a ticket (block_reduce.hpp); the last arriver goes on, with every block's count and segment visible
  if (!ticket_last_block(P.ticket, P.blocks, &wave_n[EPISODES_THREADS / 64])) return;
  const int E = P.episodes;
  const int64_t filled64 = P.counters[0];  // (read by every thread ahead of the scan's barriers; thread 0 writes it behind them)
  const int filled = filled64 < 0 ? 0 : filled64 < E ? (int)filled64 : E;
  __shared__ int32_t scan[EPISODES_THREADS];
  const int total = episode_append_offsets(P.counts, P.blocks, scan, offsets);
  for (int g = tid; g < total; g += EPISODES_THREADS) {
    const int src = episode_append_source(g, offsets, P.blocks, P.rows);
    if (g < E - filled) {  // (always, by the quotas: no store ever lands behind the list)
      const int slot = filled + g;
      P.rec_return[slot] = P.fin_return[src];
      P.rec_length[slot] = P.fin_length[src];
      P.rec_env[slot] = P.fin_env[src];
      P.rec_truncated[slot] = P.fin_truncated[src];
    }
  }
  const int new_filled = total < E - filled ? filled + total : E;
  if (tid == 0) {
    P.counters[0] = new_filled;
    if (filled < E) P.counters[1] += 1;  // steps the list needed: one that begins with a full list is not counted
  }
  if (filled == E || new_filled < E) return;  // (uniform over the block)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // the summary, in record order: the block stages EVAL_STAGE records at a time in LDS (loads in parallel), then one
  // thread adds them in order. In the second pass every square and sum rounds on its own (hipcc's default
  // -ffp-contract=fast would fuse d * d into the sum: one rounding less than the stated arithmetic; contraction is off in
  // that block only).
  __shared__ double stage_r[EVAL_STAGE];
  __shared__ int32_t stage_l[EVAL_STAGE];
  __shared__ uint8_t stage_t[EVAL_STAGE];
  double rs = 0.0, lo_r = 0.0, hi_r = 0.0;
  int64_t ls = 0, limits = 0;
  for (int k0 = 0; k0 < E; k0 += EVAL_STAGE) {
    const int cnt = min((int)EVAL_STAGE, E - k0);
    for (int k = tid; k < cnt; k += EPISODES_THREADS) {
      stage_r[k] = P.rec_return[k0 + k];
      stage_l[k] = P.rec_length[k0 + k];
      stage_t[k] = P.rec_truncated[k0 + k];
    }
    __syncthreads();
    if (tid == 0) {
      if (k0 == 0) lo_r = hi_r = stage_r[0];
#pragma unroll 8
      for (int k = 0; k < cnt; ++k) {
        const double x = stage_r[k];
        rs += x;
        ls += stage_l[k];
        limits += stage_t[k];
        lo_r = x < lo_r ? x : lo_r;
        hi_r = x > hi_r ? x : hi_r;
      }
    }
    __syncthreads();
  }
  const double n = (double)E;
  const double mean_r = rs / n, mean_l = (double)ls / n;  // (thread 0's; the others hold zeros and do not use them)
  double vr = 0.0, vl = 0.0;
  for (int k0 = 0; k0 < E; k0 += EVAL_STAGE) {
    const int cnt = min((int)EVAL_STAGE, E - k0);
    for (int k = tid; k < cnt; k += EPISODES_THREADS) {
      stage_r[k] = P.rec_return[k0 + k];
      stage_l[k] = P.rec_length[k0 + k];
    }
    __syncthreads();
    if (tid == 0) {
#pragma clang fp contract(off)
#pragma unroll 8
      for (int k = 0; k < cnt; ++k) {
        const double dr = stage_r[k] - mean_r, dl = (double)stage_l[k] - mean_l;
        const double qr = dr * dr, ql = dl * dl;
        vr = vr + qr;
        vl = vl + ql;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    P.summary[0] = mean_r;
    P.summary[1] = vr / n;
    P.summary[2] = mean_l;
    P.summary[3] = vl / n;
    P.summary[4] = lo_r;
    P.summary[5] = hi_r;
    P.summary[6] = (double)limits / n;
  }
}

__global__ __launch_bounds__(EPISODES_THREADS) void eval_reset_kernel(int num_envs, int episodes, double* ep_return, int32_t* ep_length,
                                                                    int32_t* count, int32_t* target, int64_t* counters, double* summary) {
  for (int i = blockIdx.x * EPISODES_THREADS + threadIdx.x; i < num_envs; i += gridDim.x * EPISODES_THREADS) {
    ep_return[i] = 0.0;
    ep_length[i] = 0;
    count[i] = 0;
    target[i] = (int32_t)(((int64_t)episodes + i) / num_envs);
  }
  if (blockIdx.x == 0 && threadIdx.x < EVAL_SUMMARY_WORDS) summary[threadIdx.x] = 0.0;
  if (blockIdx.x == 0 && threadIdx.x < 2) counters[threadIdx.x] = 0;
}

#endif  // __HIPCC__

}  // namespace upkie
