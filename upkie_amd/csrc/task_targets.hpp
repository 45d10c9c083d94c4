// task_targets.hpp -- the goal an env is asked to reach (a commanded ground and yaw velocity, say), drawn on the device:
// a per-env target of G words, held a random number of steps, drawn again when the hold or the episode ends, appended to
// the observation row the policy, the reward and the critic read (include/upkie_hip.h, "Task targets", states the
// arithmetic; Python: upkie_amd/targets.py). Included by upkie_hip.hip only: it needs the handle's DevConfig (seed,
// global env ids).
//
// Work split of the step and the reset: a block of TARGETS_THREADS = 256 takes TARGETS_ENVS = 16 envs. The draw is per
// env: the first 16 lanes of wave 0, lane = env, so that calls / remaining / target [g][N] are read and written with
// adjacent lanes on adjacent words; they leave the old and the current target and the end flag in LDS. Behind one barrier
// the [N][D+G] rows are written element-wise, thread i of a pass = word i of the tile's rows (a tile's rows are contiguous:
// every store of a wavefront is 256 consecutive bytes, every load contiguous up to the row seams of [N][D]). A lane per
// env walking its own row would touch 64 lines per access. 16 envs, not 64 as privileged_obs.hpp: at 4096 envs 256 blocks
// of four waves instead of 64, and a thread moves at most 16 words where it moved 64, which is what the launch's time is
// made of at wide rows; a wavefront that has no word of the tile (narrow rows) leaves behind the barrier.
//
// The curriculum is one launch of its own per PPO iteration: a block sums the scores of CURRICULUM_ENVS = 2048 envs whose
// episode count moved (thread t: envs t, t + 256, ... of the block, in that order; then block_reduce.hpp's LDS tree), the
// last block (the ticket) folds the partials in block order in fp64 and moves the limits. Fixed orders throughout and no
// float atomics: the decision is the same bits every call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "block_reduce.hpp"
#include "host_setup.hpp"

namespace upkie {

enum {
  TARGETS_THREADS = 256,
  TARGETS_ENVS = 16,
  TARGETS_MAX = UPKIE_TASK_TARGETS_MAX,
  CURRICULUM_THREADS = 256,
  CURRICULUM_ENVS = 2048,  // per block: eight per thread
};

// UpkieTaskTargets as the kernels read it (targets_params, upkie_hip.hip, checks and converts)
struct TargetsParams {
  int obs_dim, count;   // D, G
  unsigned threshold;   // every word is +0 iff (word 0 >> 8) < threshold: llround(stand_prob * 2^24)
  int steps_min;        // steps a target is held: steps_min + (word 3 >> 8) % steps_span
  unsigned steps_span;  // steps_max - steps_min + 1
  float deadband[TARGETS_MAX];
};

struct CurriculumParams {
  int count;
  double threshold;
  float step[TARGETS_MAX];
  float limit[TARGETS_MAX][2];
};

inline int curriculum_blocks(int num_envs) { return (num_envs + CURRICULUM_ENVS - 1) / CURRICULUM_ENVS; }
// the curriculum's workspace: the ticket (8 bytes, zero before the first launch), then (sum, count) fp64 per block
inline int64_t curriculum_workspace_bytes(int num_envs) { return 8 + 16 * (int64_t)curriculum_blocks(num_envs); }

// The target of (env, call) whose schedule block is r: x[g] for g < count, +0 beyond.
__device__ __forceinline__ void targets_draw(const DevConfig& C, const TargetsParams& P, const float* __restrict__ limits, unsigned lo,
                                             unsigned hi, unsigned call, const unsigned (&r)[4], float (&x)[TARGETS_MAX]) {
  const bool stand = (r[0] >> 8) < P.threshold;
#pragma unroll
  for (int blk = 0; blk < TARGETS_MAX / 4; ++blk) {
    unsigned q[4] = {0u, 0u, 0u, 0u};
    if (!stand && 4 * blk < P.count)
      philox4x32_10(lo, hi, call, ((unsigned)STREAM_TARGETS << 24) | (unsigned)(1 + blk), C.seed_lo, C.seed_hi, q);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int g = 4 * blk + i;
      float v = 0.f;
      if (!stand && g < P.count) {
        v = uniform(limits[2 * g], limits[2 * g + 1], (float)(q[i] >> 8) * (1.0f / 16777216.0f));
        if (fabsf(v) < P.deadband[g]) v = 0.f;
      }
      x[g] = v;
    }
  }
}

// The element-wise pass both kernels end with. STEP: observation and final_observation of every env of the tile; reset:
// observation of the flagged envs (final_observation is not touched). s_flag: the episode ended (step), the env is masked
// (reset). Four words per thread in flight: the loads of a pass's four iterations are issued before its stores.
template <bool STEP>
__device__ __forceinline__ void targets_write_rows(const TargetsParams& P, int env0, int envs, const float* __restrict__ next_obs,
                                                   const float* __restrict__ final_obs, const float (*s_old)[TARGETS_ENVS],
                                                   const float (*s_new)[TARGETS_ENVS], const int* s_flag, float* __restrict__ observation,
                                                   float* __restrict__ final_observation) {
  const unsigned D = (unsigned)P.obs_dim, R = (unsigned)(P.obs_dim + P.count), total = (unsigned)envs * R;
  if ((threadIdx.x & ~63u) >= total) return;  // a whole wavefront without a word of the tile
  const size_t row0 = (size_t)env0 * R;
  for (unsigned i0 = threadIdx.x; i0 < total; i0 += 4 * TARGETS_THREADS) {
    // the loads, without a branch between them: a target word also reads its env's observation word 0 (a valid address,
    // a line the row's own words bring in), an observation word also reads target word 0 from LDS; the stores select
    // (the selection is by a mask of bits: a select between two register arrays' words makes the compiler index them in scratch)
    unsigned o[4], t_new[4], t_old[4], obs_mask[4];
    size_t from[4];
    int flag[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned i = i0 + j * TARGETS_THREADS < total ? i0 + j * TARGETS_THREADS : i0;  // (a pass past the tile: word i0 again, not stored)
      const unsigned e = i / R, k = i - e * R;
      obs_mask[j] = k < D ? 0xffffffffu : 0u;
      from[j] = (size_t)(env0 + e) * D + (k & obs_mask[j]);
      o[j] = __float_as_uint(next_obs[from[j]]);
      const unsigned g = (k - D) & ~obs_mask[j];
      t_new[j] = __float_as_uint(s_new[g][e]);
      t_old[j] = __float_as_uint(s_old[g][e]);
      flag[j] = s_flag[e];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned i = i0 + j * TARGETS_THREADS;
      if (i >= total) continue;
      if (STEP) {
        float fin = __uint_as_float((o[j] & obs_mask[j]) | (t_old[j] & ~obs_mask[j]));
        if (obs_mask[j] && flag[j] && final_obs) fin = final_obs[from[j]];  // (rare: the envs whose episode ended)
        final_observation[row0 + i] = fin;
      }
      if (STEP || flag[j]) observation[row0 + i] = __uint_as_float((o[j] & obs_mask[j]) | (t_new[j] & ~obs_mask[j]));
    }
  }
}

// final_obs / terminated / truncated: each may be null (next_obs everywhere; 0).
__global__ __launch_bounds__(TARGETS_THREADS) void task_targets_kernel(DevConfig C, TargetsParams P, const float* __restrict__ next_obs,
                                                                       const float* __restrict__ final_obs,
                                                                       const uint8_t* __restrict__ terminated,
                                                                       const uint8_t* __restrict__ truncated, const float* __restrict__ limits,
                                                                       unsigned* __restrict__ calls, int* __restrict__ remaining,
                                                                       float* __restrict__ target, float* __restrict__ observation,
                                                                       float* __restrict__ final_observation) {
  __shared__ float s_old[TARGETS_MAX][TARGETS_ENVS], s_new[TARGETS_MAX][TARGETS_ENVS];
  __shared__ int s_done[TARGETS_ENVS];
  const int N = C.num_envs;
  const int env0 = blockIdx.x * TARGETS_ENVS;
  const int envs = N - env0 < TARGETS_ENVS ? N - env0 : TARGETS_ENVS;
  if ((int)threadIdx.x < envs) {
    const int n = env0 + (int)threadIdx.x;
    // the env's state, every load issued before the first wait (a word past G reads word 0 again: no branch between the loads)
    const unsigned call = calls[n];
    int left = remaining[n];
    const bool done = ((terminated ? terminated[n] : 0) | (truncated ? truncated[n] : 0)) != 0;
    float x[TARGETS_MAX];
#pragma unroll
    for (int g = 0; g < TARGETS_MAX; ++g) x[g] = target[(size_t)(g < P.count ? g : 0) * N + n];
    // 1. the call's own block: every env, every call, whatever the others do
    const unsigned lo = C.env_lo + (unsigned)n;
    const unsigned hi = C.env_hi + (lo < C.env_lo ? 1u : 0u);
    unsigned r[4];
    philox4x32_10(lo, hi, call, (unsigned)STREAM_TARGETS << 24, C.seed_lo, C.seed_hi, r);
    calls[n] = call + 1u;
    // 2. the target the policy was given: what the terminal row carries
#pragma unroll
    for (int g = 0; g < TARGETS_MAX; ++g) {
      if (g >= P.count) x[g] = 0.f;
      s_old[g][threadIdx.x] = x[g];
    }
    // 3. an ended episode ends the hold; otherwise one step of it is over
    if (done) left = 0;
    else if (left > 0) left -= 1;
    // 4. a new target
    if (left == 0) {
      left = P.steps_min + (int)((r[3] >> 8) % P.steps_span);
      targets_draw(C, P, limits, lo, hi, call, r, x);
#pragma unroll
      for (int g = 0; g < TARGETS_MAX; ++g)
        if (g < P.count) target[(size_t)g * N + n] = x[g];
    }
    remaining[n] = left;
#pragma unroll
    for (int g = 0; g < TARGETS_MAX; ++g) s_new[g][threadIdx.x] = x[g];
    s_done[threadIdx.x] = done ? 1 : 0;
  }
  __syncthreads();
  // 2. and 5. the rows
  targets_write_rows<true>(P, env0, envs, next_obs, final_obs, s_old, s_new, s_done, observation, final_observation);
}

// mask null: every env. The masked envs' draw is their call 0 and leaves calls = 1: no step draws from its blocks again.
__global__ __launch_bounds__(TARGETS_THREADS) void task_targets_reset_kernel(DevConfig C, TargetsParams P, const float* __restrict__ obs,
                                                                             const uint8_t* __restrict__ mask, const float* __restrict__ limits,
                                                                             unsigned* __restrict__ calls, int* __restrict__ remaining,
                                                                             float* __restrict__ target, float* __restrict__ observation) {
  __shared__ float s_new[TARGETS_MAX][TARGETS_ENVS];
  __shared__ int s_masked[TARGETS_ENVS];
  const int N = C.num_envs;
  const int env0 = blockIdx.x * TARGETS_ENVS;
  const int envs = N - env0 < TARGETS_ENVS ? N - env0 : TARGETS_ENVS;
  if ((int)threadIdx.x < envs) {
    const int n = env0 + (int)threadIdx.x;
    const bool masked = !mask || mask[n] != 0;
    float x[TARGETS_MAX];
#pragma unroll
    for (int g = 0; g < TARGETS_MAX; ++g) x[g] = 0.f;
    if (masked) {
      const unsigned lo = C.env_lo + (unsigned)n;
      const unsigned hi = C.env_hi + (lo < C.env_lo ? 1u : 0u);
      unsigned r[4];
      philox4x32_10(lo, hi, 0u, (unsigned)STREAM_TARGETS << 24, C.seed_lo, C.seed_hi, r);
      targets_draw(C, P, limits, lo, hi, 0u, r, x);
#pragma unroll
      for (int g = 0; g < TARGETS_MAX; ++g)
        if (g < P.count) target[(size_t)g * N + n] = x[g];
      calls[n] = 1u;
      remaining[n] = P.steps_min + (int)((r[3] >> 8) % P.steps_span);
    }
#pragma unroll
    for (int g = 0; g < TARGETS_MAX; ++g) s_new[g][threadIdx.x] = x[g];
    s_masked[threadIdx.x] = masked ? 1 : 0;
  }
  __syncthreads();
  targets_write_rows<false>(P, env0, envs, obs, nullptr, s_new, s_new, s_masked, observation, nullptr);
}

// p[0] + p[2] + ... + p[2 (grid - 1)], added in that order from 0: one fp64 word of `grid` per-block pairs, 32 loads in
// flight at a time (fold_in_block_order of block_reduce.hpp, in fp64).
__device__ __forceinline__ double fold_pairs_in_block_order(const double* p, int grid) {
  double s = 0.0;
  int b = 0;
  for (; b + 32 <= grid; b += 32) {
    double x[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) x[k] = p[2 * (size_t)(b + k)];
#pragma unroll
    for (int k = 0; k < 32; ++k) s += x[k];
  }
  for (; b < grid; ++b) s += p[2 * (size_t)b];
  return s;
}

// grid = curriculum_blocks(N). partials: [grid][2] fp64; ticket: zero before the first launch, zero after every launch.
__global__ __launch_bounds__(CURRICULUM_THREADS) void task_targets_curriculum_kernel(int N, CurriculumParams P, const double* __restrict__ score,
                                                                                     const int32_t* __restrict__ finished,
                                                                                     int32_t* __restrict__ seen, float* __restrict__ limits,
                                                                                     double* __restrict__ partials, unsigned* __restrict__ ticket) {
  __shared__ double s_sum[CURRICULUM_THREADS], s_count[CURRICULUM_THREADS];
  __shared__ int s_last;
  const int tid = (int)threadIdx.x;
  const int base = blockIdx.x * CURRICULUM_ENVS;
  double sum = 0.0, count = 0.0;
#pragma unroll
  for (int k = 0; k < CURRICULUM_ENVS / CURRICULUM_THREADS; ++k) {
    const int n = base + k * CURRICULUM_THREADS + tid;
    if (n < N) {
      const int32_t f = finished[n];
      if (f != seen[n]) {
        sum += score[n];
        count += 1.0;
        seen[n] = f;
      }
    }
  }
  s_sum[tid] = sum;
  s_count[tid] = count;
  lds_tree_sum<CURRICULUM_THREADS>(tid, s_sum, s_count);
  if (tid == 0) {
    partials[2 * (size_t)blockIdx.x] = s_sum[0];
    partials[2 * (size_t)blockIdx.x + 1] = s_count[0];
  }
  if (!ticket_last_block(ticket, (int)gridDim.x, &s_last)) return;
  if (tid != 0) return;
  const double S = fold_pairs_in_block_order(partials, (int)gridDim.x);
  const double M = fold_pairs_in_block_order(partials + 1, (int)gridDim.x);
  if (M > 0.0 && S > P.threshold * M) {
#pragma unroll
    for (int g = 0; g < TARGETS_MAX; ++g)
      if (g < P.count) {
        limits[2 * g] = fmaxf(limits[2 * g] - P.step[g], P.limit[g][0]);
        limits[2 * g + 1] = fminf(limits[2 * g + 1] + P.step[g], P.limit[g][1]);
      }
  }
}

}  // namespace upkie
