// time_limits.hpp -- Stable-Baselines3's time-limit bootstrap of collect_rollouts in ONE launch: for every env that
// ended by its time limit and not by termination (truncated && !terminated),
//   reward = fl32(reward + fl32(gamma * V(final_obs)))
// in place, two roundings and no contraction (SB3's float32 `rewards[idx] += self.gamma * terminal_value`). V is the
// critic tower of an MLP actor-critic (csrc/policy_mlp.hpp) on the final observation, normalised by the same clamp
// expression and the same packed obs_mean / obs_std words as the policy kernel: the same code on the same words, so V
// is bit for bit what upkie_mlp_actor_critic writes as the value of that observation. Only the critic runs: for an
// asymmetric shape final_obs is the critic's row [N][critic_obs_dim], with the critic's statistics block.
//
// Work split: one wave per tile of 16 envs (the policy kernel's tile; lane l holds env l & 15). The wave first reads
// its tile's flags; a tile with no env to bootstrap -- the common step: an env truncates once per max_episode_steps --
// exits before it loads a weight. Otherwise the whole tile runs the critic and only the masked envs' rewards are
// written, each by one lane (no atomics). No host argument changes between steps: the launch can be captured.
#pragma once

#include "policy_mlp.hpp"

namespace upkie {

#if defined(__HIPCC__)

template <int W, int ACT>
__global__ __launch_bounds__(64) void mlp_bootstrap_time_limits_kernel(const MlpDev P, const float* __restrict__ packed,
                                                                      const float* __restrict__ final_obs, const uint8_t* __restrict__ terminated,
                                                                      const uint8_t* __restrict__ truncated, float gamma, float* __restrict__ reward) {
  constexpr int WT = W / 16;
  const int lane = threadIdx.x, q = lane >> 4;
  const int env = blockIdx.x * 16 + (lane & 15);
  const bool valid = env < P.num_envs;
  const bool boot = valid && truncated[env] != 0 && !(terminated && terminated[env] != 0);
  if (!__any(boot)) return;  // (wave-uniform: no weight is loaded for a tile without a truncation)

  // the critic's final row (the observation's for a symmetric shape), normalised exactly as mlp_actor_critic_kernel's wave 1 does
  float x[WT][4] = {};
  const int env_c = valid ? env : P.num_envs - 1;
#pragma unroll
  for (int t = 0; t < WT; ++t) {
    if (16 * t < P.critic_obs_dim) {
      float v[4], m[4], sd[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = 16 * t + 4 * s + q, kc = k < P.critic_obs_dim ? k : P.critic_obs_dim - 1;
        v[s] = final_obs[(size_t)env_c * P.critic_obs_dim + kc];
        m[s] = packed[P.critic_mean_off + kc];
        sd[s] = packed[P.critic_std_off + kc];
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = 16 * t + 4 * s + q;
        if (valid && k < P.critic_obs_dim) {
          float u = v[s];
          if (P.normalize) u = fminf(fmaxf((u - m[s]) / sd[s], -P.clip_obs), P.clip_obs);
          x[t][s] = u;
        }
      }
    }
  }

  float head[WT][4] = {};
  float value = 0.f;
  mlp_tower<WT, ACT>(packed, P.critic, P.critic_obs_dim, x, head, &value, lane);
  if (boot && q == 0) {
    // two roundings: HIP's __fmul_rn / __fadd_rn are the plain operators, which hipcc's default -ffp-contract=fast would
    // fuse into one v_fma (one rounding, not SB3's float32 arithmetic); contraction is off in this block only
#pragma clang fp contract(off)
    const float scaled = gamma * value;
    reward[env] = reward[env] + scaled;
  }
}

#endif  // __HIPCC__

}  // namespace upkie
