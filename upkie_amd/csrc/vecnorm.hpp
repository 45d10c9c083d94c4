// vecnorm.hpp -- Stable-Baselines3's VecNormalize in training mode on the device: running mean / variance of the
// observations and of the discounted returns (RunningMeanStd, fp64), the reward scaled by the returns' running std,
// the returns of finished envs zeroed, the observations normalised -- one or two launches per env step instead of
// some 20-30 small torch ops (include/upkie_hip.h states the arithmetic; Python: upkie_amd/normalize.py).
//
// Launch A, moments (when a statistic moves: training). Block b owns envs [b R, (b + 1) R). Its 256 threads take column
// groups in turn: the observation columns, at most 256 at a time, then the column of returns alone; inside a group of
// g columns, thread t takes column t % g and rows t / g, t / g + 256 / g, ... of the block's envs, and keeps a per-lane
// (count, mean, M2) in fp64, 8 rows at a time: their loads in flight together, the 8 values reduced two-pass in
// registers, then merged in (a Welford update per chunk rather than per row, so that a lane never waits on one load per
// row). A returns lane also updates the env's return in place
// (returns = returns * gamma + reward, then 0 when the env is done). The lanes of a column are merged by Chan's formula
// in a fixed binary tree in LDS, and the block writes one partial (mean[cols], M2[cols]; its count is its number of
// envs) to the workspace. Then the ticket (block_reduce.hpp): the block that arrives last merges all partials (the same
// fixed order every call), folds the batch into the running statistics by RunningMeanStd's update and writes them in
// place with their fp32 mirrors (and a policy's packed obs_mean / obs_std words, csrc/policy_mlp.hpp).
//
// Launch B, apply (when a per-env output needs the NEW statistics: a normalised reward or normalised observations, or
// when no statistic moves). Grid-stride over envs and over observation words: reward / sqrt(ret_var + eps) in fp64,
// clipped and rounded once to fp32; (obs - mean) / std in fp32 with the fp32 mirrors, clipped -- the same expression
// as the MLP policy's, so both give the same bits; episode_starts; the returns of done envs (or all, on reset) zeroed.
// Without them (norm_reward off, no normalised observations wanted) launch A writes the per-env outputs itself and the
// step is one launch.
//
// Data-parallel form (several ranks, each with its own envs; the statistics are those of one normaliser over the union):
// launch A's last block writes this rank's batch (count, mean, M2) per column to its slot instead of folding it in; the
// caller exchanges the slots so that every rank holds every rank's row, bit for bit; launch M (merge, one block) merges
// the slots by Chan's formula in rank order, starting from slot 0 (one slot passes through unchanged), and applies the
// same RunningMeanStd update, mirrors and packed words as launch A's last block, then adds the global env count. Launch B
// follows as before. The per-env returns stay local. With one rank every output is the same bits as the fused form's.
//
// Grid of launch A: one block per 256 envs, at most 256 blocks, and at most 8192 / (2 (obs_dim + 1)) blocks so that the
// partials the last block reads stay <= 64 KB (1.4 KB at 4096 envs x 4 columns).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "block_reduce.hpp"

namespace upkie {

enum { VECNORM_THREADS = 256, VECNORM_MAX_BLOCKS = 256, VECNORM_PARTIAL_WORDS = 8192, VECNORM_PARTIALS_OFFSET = 256, VECNORM_CHUNK = 8 };

struct VecNormDev {
  int num_envs, obs_dim, packed_dp;
  int rows, blocks;         // envs per block of launch A, its grid
  int obs_cols, ret_col;    // columns launch A reduces: obs_dim (or 0), then 1 for the returns (or 0)
  int reset, norm_obs, norm_reward;
  int outputs_in_moments;   // one-launch form: launch A writes the per-env outputs
  double gamma, eps, clip_obs, clip_reward;
  const float* obs;
  const float* reward;
  const uint8_t* terminated;
  const uint8_t* truncated;
  double* obs_stats;  // mean[obs_dim], var[obs_dim], count
  double* ret_stats;  // mean, var, count
  double* returns;    // [num_envs]
  double* partials;   // [blocks][2 (obs_cols + ret_col)]
  double* slot;       // data-parallel form: this rank's slot (vecnorm_slot_doubles), or null (fused)
  unsigned* ticket;
  float* mean_f32;
  float* std_f32;
  float* packed;  // a policy's packed buffer (obs_mean at word 0, obs_std at word packed_dp) or null
  float* norm_obs_out;
  float* reward_out;
  uint8_t* starts_out;
};

// A rank's slot: n[obs_dim + 1], mean[obs_dim + 1], M2[obs_dim + 1]; column obs_dim is the returns'.
inline int vecnorm_slot_doubles(int obs_dim) { return 3 * (obs_dim + 1); }

// Grid of launch A for (num_envs, obs_dim) and its envs per block (every block owns at least one env).
inline int vecnorm_blocks(int num_envs, int obs_dim, int* rows) {
  int cap = VECNORM_PARTIAL_WORDS / (2 * (obs_dim + 1));
  cap = cap < 1 ? 1 : cap > VECNORM_MAX_BLOCKS ? VECNORM_MAX_BLOCKS : cap;
  int g = (num_envs + VECNORM_THREADS - 1) / VECNORM_THREADS;
  g = g > cap ? cap : g;
  const int r = (num_envs + g - 1) / g;
  if (rows) *rows = r;
  return (num_envs + r - 1) / r;
}

// Chan et al.'s pairwise merge of (n, mean, M2) with (nb, mb, m2b).
__device__ __forceinline__ void chan_merge(double& n, double& mean, double& m2, double nb, double mb, double m2b) {
  if (nb == 0.0) return;
  if (n == 0.0) {
    n = nb, mean = mb, m2 = m2b;
    return;
  }
  const double tot = n + nb;
  const double delta = mb - mean;
  mean += delta * (nb / tot);
  m2 += m2b + delta * delta * (n * nb / tot);
  n = tot;
}

// Merges slots 0..slots-1 of each of the `cols` columns held in LDS (n, mean, M2 of slot p, column c at index
// p * cols + c of the three 256-word arrays) into slot 0, in a fixed binary tree. Called by every thread of the block.
__device__ __forceinline__ void vecnorm_lds_tree(double* lds, int cols, int slots, int c, int p, bool active) {
  for (int live = slots; live > 1;) {
    const int half = (live + 1) >> 1;
    __syncthreads();
    if (active && p < live - half) {
      const int i = p * cols + c, j = (p + half) * cols + c;
      double n = lds[i], mean = lds[VECNORM_THREADS + i], m2 = lds[2 * VECNORM_THREADS + i];
      chan_merge(n, mean, m2, lds[j], lds[VECNORM_THREADS + j], lds[2 * VECNORM_THREADS + j]);
      lds[i] = n, lds[VECNORM_THREADS + i] = mean, lds[2 * VECNORM_THREADS + i] = m2;
    }
    live = half;
  }
  __syncthreads();
}

__device__ __forceinline__ bool vecnorm_done(const VecNormDev& P, int r) {
  return (P.terminated && P.terminated[r]) || (P.truncated && P.truncated[r]);
}

// The per-env outputs of env r: episode start, reward (normalised by `ret_scale` = 1 / sqrt(ret_var + eps) in fp64
// when norm_reward), and the returns zeroed on reset or when done.
__device__ __forceinline__ void vecnorm_env(const VecNormDev& P, int r, double ret_std) {
  const bool done = vecnorm_done(P, r);
  if (P.starts_out) P.starts_out[r] = done ? 1 : 0;
  if (P.reward_out) {
    const double x = (double)P.reward[r];
    P.reward_out[r] = P.norm_reward ? (float)fmin(fmax(x / ret_std, -P.clip_reward), P.clip_reward) : (float)x;
  }
  if (P.reset || done) P.returns[r] = 0.0;
}

// Adds the values of rows first, first + step, ... < end of one lane to its (n, mean, M2): VECNORM_CHUNK rows at a time,
// their loads issued together (a row past the end loads row `first` again and is not counted: no branch around a
// load), each chunk reduced two-pass in registers and merged by Chan's formula. `load(r)` reads row r's value,
// `flag(r)` one more bit of it; `keep(r, x, flag)` is called for the counted rows after the chunk's loads (the returns
// column writes the updated return back there).
template <class Load, class Flag, class Keep>
__device__ __forceinline__ void vecnorm_lane_moments(int first, int end, int step, Load load, Flag flag, Keep keep, double& n, double& mean,
                                                     double& m2) {
  for (int r0 = first; r0 < end; r0 += VECNORM_CHUNK * step) {
    double x[VECNORM_CHUNK];
    bool f[VECNORM_CHUNK];
#pragma unroll
    for (int j = 0; j < VECNORM_CHUNK; ++j) {
      const int r = r0 + j * step < end ? r0 + j * step : first;
      x[j] = load(r);
      f[j] = flag(r);
    }
    const int count = min((int)VECNORM_CHUNK, (end - r0 + step - 1) / step);
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < VECNORM_CHUNK; ++j) sum += j < count ? x[j] : 0.0;
    const double cm = sum / count;
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < VECNORM_CHUNK; ++j) {
      const double d = j < count ? x[j] - cm : 0.0;
      q += d * d;
      if (j < count) keep(r0 + j * step, x[j], f[j]);
    }
    chan_merge(n, mean, m2, (double)count, cm, q);
  }
}

// RunningMeanStd.update_from_moments of column `col` (an observation column below obs_cols, else the returns) with the
// batch (count bn, mean bm, M2 = var * count bm2), in place, with the fp32 mirrors and a policy's packed words. The
// counts themselves move after every column has read them.
__device__ __forceinline__ void vecnorm_update_column(const VecNormDev& P, int col, double bn, double bm, double bm2) {
  const int D = P.obs_dim;
  const bool is_obs = col < P.obs_cols;
  double* mean_p = is_obs ? P.obs_stats + col : P.ret_stats;
  double* var_p = is_obs ? P.obs_stats + D + col : P.ret_stats + 1;
  const double count = is_obs ? P.obs_stats[2 * D] : P.ret_stats[2];
  const double old_mean = *mean_p, old_var = *var_p;
  const double delta = bm - old_mean, tot = count + bn;
  const double new_mean = old_mean + delta * bn / tot;
  const double new_var = (old_var * count + bm2 + delta * delta * count * bn / tot) / tot;
  *mean_p = new_mean;
  *var_p = new_var;
  if (is_obs) {
    const float m32 = (float)new_mean, s32 = (float)sqrt(new_var + P.eps);
    P.mean_f32[col] = m32;
    P.std_f32[col] = s32;
    if (P.packed) P.packed[col] = m32, P.packed[P.packed_dp + col] = s32;
  }
}

__global__ __launch_bounds__(VECNORM_THREADS) void vecnorm_moments_kernel(const VecNormDev P) {
  __shared__ double lds[3 * VECNORM_THREADS + 1];  // n, mean, M2 per thread; [3 * 256]: "last block" flag
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * P.rows, r1 = min(P.num_envs, r0 + P.rows);
  const int cols = P.obs_cols + P.ret_col;
  double* part = P.partials + (size_t)blockIdx.x * 2 * cols;

  // column groups: the observation columns, at most 256 at a time, then the returns column alone (no lane of a group
  // branches differently from another around its loads)
  for (int c0 = 0; c0 < cols;) {
    const bool returns = c0 >= P.obs_cols;
    const int g = returns ? 1 : min(P.obs_cols - c0, (int)VECNORM_THREADS), slots = VECNORM_THREADS / g;
    const int c = c0 + tid % g, p = tid / g;
    const bool active = p < slots;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    if (active) {
      if (returns)
        vecnorm_lane_moments(
            r0 + p, r1, slots, [&](int r) { return P.returns[r] * P.gamma + (double)P.reward[r]; }, [&](int r) { return vecnorm_done(P, r); },
            [&](int r, double x, bool done) { P.returns[r] = done ? 0.0 : x; }, n, mean, m2);
      else
        vecnorm_lane_moments(
            r0 + p, r1, slots, [&](int r) { return (double)P.obs[(size_t)r * P.obs_dim + c]; }, [](int) { return false; },
            [](int, double, bool) {}, n, mean, m2);
      lds[tid] = n, lds[VECNORM_THREADS + tid] = mean, lds[2 * VECNORM_THREADS + tid] = m2;  // (slot p, column c: p g + c - c0 = tid)
    }
    vecnorm_lds_tree(lds, g, slots, tid % g, p, active);
    if (tid < g) part[c0 + tid] = lds[VECNORM_THREADS + tid], part[cols + c0 + tid] = lds[2 * VECNORM_THREADS + tid];
    __syncthreads();
    c0 += g;
  }

  if (P.outputs_in_moments) {
    const double ret_std = P.norm_reward ? sqrt(P.ret_stats[1] + P.eps) : 1.0;  // (one-launch form: norm_reward is off)
    for (int r = r0 + tid; r < r1; r += VECNORM_THREADS) vecnorm_env(P, r, ret_std);
  }

  // publish the partial and draw a ticket (block_reduce.hpp); the last arriver goes on, with every partial visible
  if (!ticket_last_block(P.ticket, P.blocks, &lds[3 * VECNORM_THREADS])) return;
  const int D = P.obs_dim;
  for (int c0 = 0; c0 < cols; c0 += VECNORM_THREADS) {
    const int g = min(cols - c0, (int)VECNORM_THREADS), slots = min(P.blocks, VECNORM_THREADS / g);
    const int c = c0 + tid % g, p = tid / g;
    const bool active = p < slots;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    if (active) {
      for (int b = p; b < P.blocks; b += slots) {  // (partials p, p + slots, ...: a fixed order)
        const double* pb = P.partials + (size_t)b * 2 * cols;
        chan_merge(n, mean, m2, (double)(min(P.num_envs, (b + 1) * P.rows) - b * P.rows), pb[c], pb[cols + c]);
      }
      lds[tid] = n, lds[VECNORM_THREADS + tid] = mean, lds[2 * VECNORM_THREADS + tid] = m2;
    }
    vecnorm_lds_tree(lds, g, slots, tid % g, p, active);
    if (tid < g) {
      const int col = c0 + tid;
      const double bn = lds[tid], bm = lds[VECNORM_THREADS + tid], bm2 = lds[2 * VECNORM_THREADS + tid];
      if (P.slot) {
        const int sc = col < P.obs_cols ? col : D;
        P.slot[sc] = bn, P.slot[D + 1 + sc] = bm, P.slot[2 * (D + 1) + sc] = bm2;
      } else {
        vecnorm_update_column(P, col, bn, bm, bm2);
      }
    }
    __syncthreads();
  }
  if (P.slot) return;
  if (tid == 0) {  // (after every column read the old counts)
    if (P.obs_cols) P.obs_stats[2 * D] += (double)P.num_envs;
    if (P.ret_col) P.ret_stats[2] += (double)P.num_envs;
  }
}

// Launch M (data-parallel form, one block): Chan's merge of the `world` exchanged slots (stride doubles apart) in rank
// order from slot 0, per column launch A reduces, then the update of launch A's last block; the counts grow by the
// merged env count.
__global__ __launch_bounds__(VECNORM_THREADS) void vecnorm_merge_kernel(const VecNormDev P, const double* __restrict__ slots, int world, int stride) {
  const int D = P.obs_dim, tid = threadIdx.x;
  const int cols = P.obs_cols + P.ret_col;
  auto merged = [&](int sc, double& n, double& mean, double& m2) {
    n = slots[sc], mean = slots[D + 1 + sc], m2 = slots[2 * (D + 1) + sc];
    for (int r = 1; r < world; ++r) {
      const double* q = slots + (size_t)r * stride;
      chan_merge(n, mean, m2, q[sc], q[D + 1 + sc], q[2 * (D + 1) + sc]);
    }
  };
  for (int col = tid; col < cols; col += VECNORM_THREADS) {
    double n, mean, m2;
    merged(col < P.obs_cols ? col : D, n, mean, m2);
    vecnorm_update_column(P, col, n, mean, m2);
  }
  __syncthreads();
  if (tid == 0) {  // (after every column read the old counts)
    double n, mean, m2;
    if (P.obs_cols) merged(0, n, mean, m2), P.obs_stats[2 * D] += n;
    if (P.ret_col) merged(D, n, mean, m2), P.ret_stats[2] += n;
  }
}

__global__ __launch_bounds__(VECNORM_THREADS) void vecnorm_apply_kernel(const VecNormDev P) {
  const int stride = gridDim.x * VECNORM_THREADS;
  const int i0 = blockIdx.x * VECNORM_THREADS + threadIdx.x;
  const double ret_std = P.norm_reward && P.reward_out ? sqrt(P.ret_stats[1] + P.eps) : 1.0;
  for (int r = i0; r < P.num_envs; r += stride) vecnorm_env(P, r, ret_std);
  if (P.norm_obs_out) {
    const int D = P.obs_dim, words = P.num_envs * D;
    const float clip = (float)P.clip_obs;
    for (int i = i0; i < words; i += stride) {
      float u = P.obs[i];
      if (P.norm_obs) {
        const int d = i % D;
        u = fminf(fmaxf((u - P.mean_f32[d]) / P.std_f32[d], -clip), clip);
      }
      P.norm_obs_out[i] = u;
    }
  }
}

}  // namespace upkie
