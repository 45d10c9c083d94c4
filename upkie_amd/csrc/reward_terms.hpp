// reward_terms.hpp -- a declarative reward of up to 16 weighted terms for a batch of envs, in ONE launch per env step:
// the reward itself (read from the terminal observation where an episode ended), the action the rate terms of the next
// step compare with, and per env and per term the fp64 sum of the running episode and of the last finished one
// (include/upkie_hip.h states the arithmetic; Python: upkie_amd/rewards.py).
//
// Work split: one lane serves one env, blocks of 256, no LDS, no atomics, no block that reads what another writes: the
// same bits every call and under graph replay.
//
// The term table (RewardTable: sizes, 1/dt, the clamp, and per term its shape, weight, scale and taps) is packed and
// checked once on the host (upkie_reward_terms_params) and lives in a small device block. Every lane of a launch reads
// the same table words, so it is reached through the constant address space: the loads are scalar loads, the loops over
// terms and taps and the switches on a tap's source, function and a term's shape are scalar branches, and no lane
// diverges from another but for the flags of its env. A table packed for other sizes than the launch's (or a block that is
// no table) makes the launch do nothing rather than index out of bounds.
//
// Layout of the per-env state, struct-of-arrays so that every state access of a wavefront is contiguous:
//   term_sum, term_last [K][N] fp64: lane e touches word k N + e, a wavefront 512 contiguous bytes per term;
//   prev_action [A][N] float32: word j N + e, 256 contiguous bytes per action word. ([N][A], the caller's layout of
//     `action`, would make every access of a rate tap a stride-A gather; the action itself is read in that layout
//     because the policy and the pipeline write it so.)
//   finished [N] int32.
//
// Loads: the flags first. An observation row of exactly 4 words on 16-byte aligned buffers is ONE 16-byte load per lane
// and row (the next and the final row are both issued before the flags are back, then selected); rows of 1-3 words (and
// 4-word rows of a buffer that is not 16-byte aligned) are read word by word from the row the flags select; wider rows
// load only the tapped words, from that row.
// Per term the fp64 sum and every tap's words (up to 8, action and previous action of a rate tap) are issued before
// the first arithmetic that depends on one of them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/upkie_hip.h"

namespace upkie {

enum { REWARD_THREADS = 256, REWARD_MAGIC = 0x52575431 };

struct RewardTap {
  int32_t source, index, fn;  // UpkieRewardSource, the word of the source, UpkieRewardFn
  float coef;
};

struct RewardTerm {
  int32_t shape, num_taps;  // UpkieRewardShape, 1-8
  float weight, scale;
  RewardTap taps[UPKIE_REWARD_MAX_TAPS];
};

struct RewardTable {
  int32_t magic, num_terms, obs_dim, act_dim;
  float inv_dt, clip_low, clip_high;
  int32_t reserved;
  RewardTerm terms[UPKIE_REWARD_MAX_TERMS];
};

static_assert(sizeof(RewardTable) == UPKIE_REWARD_PARAMS_BYTES, "the packed term table is UPKIE_REWARD_PARAMS_BYTES long");

struct RewardDev {
  int num_envs, obs_dim, act_dim, num_terms;
  int row16;  // obs_dim == 4 and both observation buffers 16-byte aligned: one 16-byte load per row
  const void* table;
  const float* next_obs;
  const float* action;
  const uint8_t* terminated;
  const uint8_t* truncated;
  const float* final_obs;
  float* prev_action;  // [A][N]
  double* term_sum;    // [K][N]
  double* term_last;   // [K][N]
  int32_t* finished;   // [N]
  float* reward;       // [N]
};

#if defined(__HIPCC__)

__global__ __launch_bounds__(REWARD_THREADS) void reward_terms_step_kernel(const RewardDev P) {
  // the products, sums and differences below round one by one (hipcc's default -ffp-contract=fast would fuse w * y
  // into the reward's sum: one rounding less, 1 ulp off the stated arithmetic on some envs); fmaf stays a fused multiply-add
#pragma clang fp contract(off)
  typedef const __attribute__((address_space(4))) RewardTable* ConstTable;
  const ConstTable T = (ConstTable)P.table;
  const int N = P.num_envs, D = P.obs_dim, A = P.act_dim, K = P.num_terms;
  if (T->magic != REWARD_MAGIC || T->num_terms != K || T->obs_dim != D || T->act_dim != A) return;
  const int e = blockIdx.x * REWARD_THREADS + threadIdx.x;
  if (e >= N) return;

  const bool has_final = P.final_obs != nullptr;
  float o[4] = {0.f, 0.f, 0.f, 0.f};
  float4 row_next = {0.f, 0.f, 0.f, 0.f}, row_final = {0.f, 0.f, 0.f, 0.f};
  if (P.row16) {
    row_next = reinterpret_cast<const float4*>(P.next_obs)[e];
    if (has_final) row_final = reinterpret_cast<const float4*>(P.final_obs)[e];
  }
  const bool terminated = P.terminated && P.terminated[e] != 0;
  const bool ended = terminated || (P.truncated && P.truncated[e] != 0);
  const bool terminal_row = ended && has_final;
  const float* row = (terminal_row ? P.final_obs : P.next_obs) + (size_t)e * D;
  const float* act = P.action + (size_t)e * A;
  const float* prev = P.prev_action + e;
  if (P.row16) {
    const float4 r = terminal_row ? row_final : row_next;
    o[0] = r.x, o[1] = r.y, o[2] = r.z, o[3] = r.w;
  } else if (D <= 4) {
    o[0] = row[0];
    if (D > 1) o[1] = row[1];
    if (D > 2) o[2] = row[2];
    if (D > 3) o[3] = row[3];
  }
  const bool in_registers = D <= 4;
  const float inv_dt = T->inv_dt;
  const float flag_terminated = terminated ? 1.f : 0.f;

  float reward = 0.f;
  for (int k = 0; k < K; ++k) {
    const size_t at = (size_t)k * N + e;
    const double sum_before = P.term_sum[at];
    const int n = T->terms[k].num_taps;
    float va[UPKIE_REWARD_MAX_TAPS], vb[UPKIE_REWARD_MAX_TAPS];
#pragma unroll
    for (int j = 0; j < UPKIE_REWARD_MAX_TAPS; ++j) {
      va[j] = 0.f, vb[j] = 0.f;
      if (j < n) {
        const int source = T->terms[k].taps[j].source, index = T->terms[k].taps[j].index;
        if (source == UPKIE_REWARD_OBS) {
          if (in_registers) va[j] = index == 0 ? o[0] : index == 1 ? o[1] : index == 2 ? o[2] : o[3];
          else va[j] = row[index];
        } else if (source == UPKIE_REWARD_ACTION) {
          va[j] = act[index];
        } else if (source == UPKIE_REWARD_ACTION_RATE) {
          va[j] = act[index];
          vb[j] = prev[(size_t)index * N];
        } else if (source == UPKIE_REWARD_ONE) {
          va[j] = 1.f;
        } else {
          va[j] = flag_terminated;
        }
      }
    }
    float x = 0.f;
#pragma unroll
    for (int j = 0; j < UPKIE_REWARD_MAX_TAPS; ++j) {
      if (j < n) {
        const int source = T->terms[k].taps[j].source, fn = T->terms[k].taps[j].fn;
        float v = va[j];
        if (source == UPKIE_REWARD_ACTION_RATE) {
          const float diff = va[j] - vb[j];
          v = diff * inv_dt;
        }
        if (fn == UPKIE_REWARD_FN_SIN) v = sinf(v);
        else if (fn == UPKIE_REWARD_FN_COS) v = cosf(v);
        x = fmaf(T->terms[k].taps[j].coef, v, x);
      }
    }
    const int shape = T->terms[k].shape;
    const float s = T->terms[k].scale;
    float y = x;
    if (shape == UPKIE_REWARD_ABS) {
      y = fabsf(x);
    } else if (shape == UPKIE_REWARD_SQUARE) {
      y = x * x;
    } else if (shape == UPKIE_REWARD_EXP_ABS) {
      const float q = fabsf(x) / s;
      y = expf(-q);
    } else if (shape == UPKIE_REWARD_EXP_SQUARE) {
      const float q = x / s;
      const float q2 = q * q;
      y = expf(-q2);
    } else if (shape == UPKIE_REWARD_DEADBAND) {
      const float t = fabsf(x) - s;
      y = t < 0.f ? 0.f : t;  // (a NaN passes)
    }
    const float v = T->terms[k].weight * y;
    reward = reward + v;
    const double sum = sum_before + (double)v;
    if (ended) P.term_last[at] = sum;
    P.term_sum[at] = ended ? 0.0 : sum;
  }
  const float lo = T->clip_low, hi = T->clip_high;
  P.reward[e] = reward < lo ? lo : (reward > hi ? hi : reward);  // (a NaN passes; infinite bounds never bind)
  if (ended) P.finished[e] += 1;
  for (int j = 0; j < A; ++j) {
    const float a = act[j];
    P.prev_action[(size_t)j * N + e] = ended ? 0.f : a;
  }
}

__global__ __launch_bounds__(REWARD_THREADS) void reward_terms_reset_kernel(int num_envs, int act_dim, int num_terms,
                                                                            const uint8_t* __restrict__ mask, float* prev_action,
                                                                            double* term_sum) {
  const int e = blockIdx.x * REWARD_THREADS + threadIdx.x;
  if (e >= num_envs || (mask && mask[e] == 0)) return;
  for (int k = 0; k < num_terms; ++k) term_sum[(size_t)k * num_envs + e] = 0.0;
  for (int j = 0; j < act_dim; ++j) prev_action[(size_t)j * num_envs + e] = 0.f;
}

#endif  // __HIPCC__

}  // namespace upkie
