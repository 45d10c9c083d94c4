// trainer_abi.hip -- handle-free entry points of include/upkie_hip.h around a rollout: the MLP actor-critic policy, the
// time-limit bootstrap, episode statistics, the evaluation tally, the agent pipeline, the reward terms, the privileged
// observation, VecNormalize, the linear policy and GAE. Host code around the kernels of the headers below; nothing here
// takes or touches a simulator, MPC or observer handle (upkie_hip.hip). The PPO update, the other heavy set of kernel
// instantiations, is ppo_abi.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "mlp_instances.hpp"
#include "rollout.hpp"
#include "vecnorm.hpp"
#include "time_limits.hpp"
#include "episodes.hpp"
#include "eval_episodes.hpp"
#include "agent_pipeline.hpp"
#include "reward_terms.hpp"
#include "privileged_obs.hpp"

#include "abi_host.hpp"

// ============================================================ MLP actor-critic policy
extern "C" int64_t upkie_mlp_packed_words(const UpkieMlpShape* shape) {
  if (!shape) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null shape");
  const int64_t words = upkie::mlp_layout(*shape, nullptr);
  if (words >= 0) return words;
  return fail(UPKIE_ERR_INVALID_ARGUMENT,
              "MLP shape out of range (obs_dim 1-256, act_dim 1-64, 1-4 actor / 0-4 critic layers of 1-256 units, tanh or relu, clip_obs > 0, "
              "critic_obs_dim 0 or 1-256 with a critic)");
}

// upkie_mlp_actor_critic (critic_obs = obs, no norm_critic_obs) and upkie_mlp_actor_critic_asym: one launch.
static int mlp_actor_critic(int32_t num_envs, const UpkieMlpShape* shape, const float* packed, const float* obs, const float* critic_obs,
                            uint32_t* calls, uint64_t seed, int32_t deterministic, float* norm_obs, float* norm_critic_obs, float* mean,
                            float* action, float* env_action, float* value, float* log_prob, void* stream) {
  if (num_envs <= 0) return fail(UPKIE_ERR_INVALID_ARGUMENT, "num_envs must be positive");
  if (!shape || !packed || !obs) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument");
  if (!critic_obs && (value || norm_critic_obs)) return fail(UPKIE_ERR_INVALID_ARGUMENT, "value and norm_critic_obs need critic_obs");
  upkie::MlpDev P;
  if (upkie::mlp_layout(*shape, &P) < 0)
    return (int)upkie_mlp_packed_words(shape);  // (sets the message)
  P.num_envs = num_envs;
  P.run_actor = mean || action || env_action || log_prob;
  P.run_critic = value != nullptr;
  P.sample = P.run_actor && !deterministic;
  if (P.run_critic && shape->critic_layers == 0) return fail(UPKIE_ERR_INVALID_ARGUMENT, "a value output needs a critic (critic_layers > 0)");
  if (P.sample && !calls) return fail(UPKIE_ERR_INVALID_ARGUMENT, "sampling needs the per-env call counters");
  P.seed_lo = (unsigned)(seed & 0xffffffffu);
  P.seed_hi = (unsigned)(seed >> 32);
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  if (!P.run_actor && !P.run_critic && !norm_obs && !norm_critic_obs) return UPKIE_OK;
  const upkie::MlpOutputs out{norm_obs, norm_critic_obs, mean, action, env_action, value, log_prob};
  const dim3 grid((unsigned)((num_envs + 15) / 16));
  for_mlp_instance(*shape, [&](auto w, auto act) {
    hipLaunchKernelGGL((upkie::mlp_actor_critic_kernel<w(), act()>), grid, dim3(128), 0, (hipStream_t)stream, P, packed, obs, critic_obs, calls,
                       out);
  });
  return launch_status();
}

static int refuse_asymmetric(const UpkieMlpShape* shape, const char* entry, const char* other) {
  if (shape && shape->critic_obs_dim != 0)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, std::string(entry) + ": the shape is asymmetric (critic_obs_dim " +
                                                std::to_string(shape->critic_obs_dim) + ", obs_dim " + std::to_string(shape->obs_dim) +
                                                "): the critic's rows go to " + other);
  return UPKIE_OK;
}

extern "C" int upkie_mlp_actor_critic(int32_t num_envs, const UpkieMlpShape* shape, const float* packed, const float* obs, uint32_t* calls,
                                      uint64_t seed, int32_t deterministic, float* norm_obs, float* mean, float* action, float* env_action,
                                      float* value, float* log_prob, void* stream) {
  if (refuse_asymmetric(shape, "upkie_mlp_actor_critic", "upkie_mlp_actor_critic_asym")) return UPKIE_ERR_INVALID_ARGUMENT;
  return mlp_actor_critic(num_envs, shape, packed, obs, obs, calls, seed, deterministic, norm_obs, nullptr, mean, action, env_action, value,
                          log_prob, stream);
}

extern "C" int upkie_mlp_actor_critic_asym(int32_t num_envs, const UpkieMlpShape* shape, const float* packed, const float* obs,
                                           const float* critic_obs, uint32_t* calls, uint64_t seed, int32_t deterministic, float* norm_obs,
                                           float* norm_critic_obs, float* mean, float* action, float* env_action, float* value,
                                           float* log_prob, void* stream) {
  return mlp_actor_critic(num_envs, shape, packed, obs, critic_obs, calls, seed, deterministic, norm_obs, norm_critic_obs, mean, action,
                          env_action, value, log_prob, stream);
}

// ============================================================ time-limit bootstrap (SB3 collect_rollouts)
extern "C" int upkie_mlp_bootstrap_time_limits(int32_t num_envs, const UpkieMlpShape* shape, const float* packed, const float* final_obs,
                                               const uint8_t* terminated, const uint8_t* truncated, double gamma, float* reward, void* stream) {
  if (num_envs <= 0) return fail(UPKIE_ERR_INVALID_ARGUMENT, "num_envs must be positive");
  if (!shape || !packed || !final_obs || !truncated || !reward)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument (shape, packed, final_obs, truncated and reward are required)");
  upkie::MlpDev P;
  if (upkie::mlp_layout(*shape, &P) < 0)
    return (int)upkie_mlp_packed_words(shape);  // (sets the message)
  if (shape->critic_layers == 0) return fail(UPKIE_ERR_INVALID_ARGUMENT, "the time-limit bootstrap needs a critic (critic_layers > 0)");
  if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(UPKIE_ERR_INVALID_ARGUMENT, "gamma must be in [0, 1]");
  P.num_envs = num_envs;
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  const dim3 grid((unsigned)((num_envs + 15) / 16));
  const float g32 = (float)gamma;
  for_mlp_instance(*shape, [&](auto w, auto act) {
    hipLaunchKernelGGL((upkie::mlp_bootstrap_time_limits_kernel<w(), act()>), grid, dim3(64), 0, (hipStream_t)stream, P, packed, final_obs,
                       terminated, truncated, g32, reward);
  });
  return launch_status();
}

// ============================================================ episode statistics (SB3 Monitor + ep_info_buffer)
static int check_episodes_shape(int32_t num_envs, int32_t window) {
  if (num_envs <= 0 || window < 1 || window > upkie::EPISODES_MAX_WINDOW)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "num_envs must be positive and window in 1-65536");
  return UPKIE_OK;
}

extern "C" int64_t upkie_episodes_workspace_bytes(int32_t num_envs) {
  if (check_episodes_shape(num_envs, 1)) return UPKIE_ERR_INVALID_ARGUMENT;
  return upkie::episodes_workspace_bytes(num_envs);
}

extern "C" int upkie_episodes_step(int32_t num_envs, int32_t window, const float* reward, const uint8_t* terminated, const uint8_t* truncated,
                                   double* ep_return, int32_t* ep_length, double* ring_return, int32_t* ring_length, int64_t* counters,
                                   double* means, void* workspace, void* stream) {
  if (check_episodes_shape(num_envs, window)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!reward || !ep_return || !ep_length || !ring_return || !ring_length || !counters || !means || !workspace)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument (only terminated and truncated may be NULL)");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  upkie::EpisodesDev P{};
  P.num_envs = num_envs, P.window = window;
  P.blocks = upkie::episodes_blocks(num_envs, &P.rows);
  P.reward = reward, P.terminated = terminated, P.truncated = truncated;
  P.ep_return = ep_return, P.ep_length = ep_length, P.ring_return = ring_return, P.ring_length = ring_length;
  P.counters = counters, P.means = means;
  const upkie::EpisodeAppendWorkspace ws = upkie::episode_append_carve(workspace, num_envs);
  P.ticket = ws.ticket, P.counts = ws.counts, P.fin_return = ws.segment<double>(0), P.fin_length = ws.segment<int32_t>(8);
  hipLaunchKernelGGL(upkie::episodes_step_kernel, dim3((unsigned)P.blocks), dim3(upkie::EPISODES_THREADS), 0, (hipStream_t)stream, P);
  return launch_status();
}

extern "C" int upkie_episodes_reset(int32_t num_envs, const uint8_t* mask, double* ep_return, int32_t* ep_length, void* stream) {
  if (check_episodes_shape(num_envs, 1)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!ep_return || !ep_length) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null accumulator buffer");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  const int grid = upkie::episodes_reset_blocks(num_envs);
  hipLaunchKernelGGL(upkie::episodes_reset_kernel, dim3((unsigned)grid), dim3(upkie::EPISODES_THREADS), 0, (hipStream_t)stream, num_envs, mask,
                     ep_return, ep_length);
  return launch_status();
}

// ============================================================ evaluation tally (SB3 evaluate_policy's bookkeeping)
static int check_eval_shape(int32_t num_envs, int32_t capacity, int32_t n_eval_episodes) {
  if (num_envs <= 0 || capacity < 1) return fail(UPKIE_ERR_INVALID_ARGUMENT, "eval: num_envs and capacity must be positive");
  if (n_eval_episodes < 1 || n_eval_episodes > capacity)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "eval: n_eval_episodes must be in 1-capacity (the record buffers hold `capacity` entries)");
  return UPKIE_OK;
}

extern "C" int64_t upkie_eval_workspace_bytes(int32_t num_envs) {
  if (check_eval_shape(num_envs, 1, 1)) return UPKIE_ERR_INVALID_ARGUMENT;
  return upkie::eval_workspace_bytes(num_envs);
}

extern "C" int upkie_eval_reset(int32_t num_envs, int32_t capacity, int32_t n_eval_episodes, double* ep_return, int32_t* ep_length,
                                int32_t* count, int32_t* target, int64_t* counters, double* summary, void* stream) {
  if (check_eval_shape(num_envs, capacity, n_eval_episodes)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!ep_return || !ep_length || !count || !target || !counters || !summary) return fail(UPKIE_ERR_INVALID_ARGUMENT, "eval: null state buffer");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  const int grid = upkie::episodes_reset_blocks(num_envs);
  hipLaunchKernelGGL(upkie::eval_reset_kernel, dim3((unsigned)grid), dim3(upkie::EPISODES_THREADS), 0, (hipStream_t)stream, num_envs,
                     n_eval_episodes, ep_return, ep_length, count, target, counters, summary);
  return launch_status();
}

extern "C" int upkie_eval_step(int32_t num_envs, int32_t capacity, int32_t n_eval_episodes, const float* reward, const uint8_t* terminated,
                               const uint8_t* truncated, double* ep_return, int32_t* ep_length, int32_t* count, const int32_t* target,
                               double* rec_return, int32_t* rec_length, int32_t* rec_env, uint8_t* rec_truncated, int64_t* counters,
                               double* summary, void* workspace, void* stream) {
  if (check_eval_shape(num_envs, capacity, n_eval_episodes)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!reward || !ep_return || !ep_length || !count || !target || !rec_return || !rec_length || !rec_env || !rec_truncated || !counters ||
      !summary || !workspace)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "eval: null argument (only terminated and truncated may be NULL)");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  upkie::EvalDev P{};
  P.num_envs = num_envs, P.episodes = n_eval_episodes;
  P.blocks = upkie::episodes_blocks(num_envs, &P.rows);
  P.reward = reward, P.terminated = terminated, P.truncated = truncated;
  P.ep_return = ep_return, P.ep_length = ep_length, P.count = count, P.target = target;
  P.rec_return = rec_return, P.rec_length = rec_length, P.rec_env = rec_env, P.rec_truncated = rec_truncated;
  P.counters = counters, P.summary = summary;
  const upkie::EpisodeAppendWorkspace ws = upkie::episode_append_carve(workspace, num_envs);
  P.ticket = ws.ticket, P.counts = ws.counts, P.fin_return = ws.segment<double>(0), P.fin_length = ws.segment<int32_t>(8);
  P.fin_env = ws.segment<int32_t>(12), P.fin_truncated = ws.segment<uint8_t>(16);
  hipLaunchKernelGGL(upkie::eval_step_kernel, dim3((unsigned)P.blocks), dim3(upkie::EPISODES_THREADS), 0, (hipStream_t)stream, P);
  return launch_status();
}

// ============================================================ agent pipeline (action shaping, noise, VecFrameStack)
extern "C" int64_t upkie_pipeline_params(int32_t obs_dim, int32_t act_dim, const float* action_low, const float* action_high,
                                         const float* action_noise, const float* observation_noise, float* params) {
  if (obs_dim < 1 || obs_dim > 256 || act_dim < 1 || act_dim > 64)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: obs_dim must be in 1-256 and act_dim in 1-64");
  if (!action_low || !action_high) return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: null action bounds");
  for (int a = 0; a < act_dim; ++a)
    if (!(action_low[a] <= action_high[a])) return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: action bounds need low <= high (and no NaN)");
  for (int a = 0; action_noise && a < act_dim; ++a)
    if (!(action_noise[a] >= 0.f) || !std::isfinite(action_noise[a]))
      return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: action_noise sigmas must be non-negative and finite");
  for (int d = 0; observation_noise && d < obs_dim; ++d)
    if (!(observation_noise[d] >= 0.f) || !std::isfinite(observation_noise[d]))
      return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: observation_noise sigmas must be non-negative and finite");
  if (params) {
    for (int a = 0; a < act_dim; ++a) {
      params[a] = action_low[a];
      params[act_dim + a] = action_high[a];
      params[2 * act_dim + a] = action_noise ? action_noise[a] : 0.f;
    }
    for (int d = 0; d < obs_dim; ++d) params[3 * act_dim + d] = observation_noise ? observation_noise[d] : 0.f;
  }
  return 3 * (int64_t)act_dim + obs_dim;
}

// The settings every pipeline launch begins with, checked; UPKIE_OK or the error status (message set).
static int pipeline_setup(int32_t num_envs, int32_t obs_dim, int32_t act_dim, int32_t stack, int32_t flags, double dt, double action_lag,
                          const float* params, uint64_t seed, upkie::PipelineDev* out) {
  const int32_t known = UPKIE_PIPELINE_ACTION_IN_OBSERVATION | UPKIE_PIPELINE_INTEGRATE_ACTION | UPKIE_PIPELINE_ACTION_NOISE |
                        UPKIE_PIPELINE_ACTION_LAG | UPKIE_PIPELINE_OBSERVATION_NOISE;
  if (num_envs <= 0 || num_envs > INT_MAX / upkie::PIPELINE_WAVE_WORDS)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: num_envs must be positive (and num_envs * 256 below 2^31)");
  if (flags & ~known) return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: unknown flags");
  upkie::PipelineDev P{};
  P.num_envs = num_envs, P.obs_dim = obs_dim, P.act_dim = act_dim, P.stack = stack;
  P.action_in_obs = (flags & UPKIE_PIPELINE_ACTION_IN_OBSERVATION) != 0;
  P.integrate = (flags & UPKIE_PIPELINE_INTEGRATE_ACTION) != 0;
  P.action_noise = (flags & UPKIE_PIPELINE_ACTION_NOISE) != 0;
  P.lag = (flags & UPKIE_PIPELINE_ACTION_LAG) != 0;
  P.obs_noise = (flags & UPKIE_PIPELINE_OBSERVATION_NOISE) != 0;
  if (stack < 1) return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: stack must be at least 1");
  if (act_dim < 1 || act_dim > 64) return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: act_dim must be in 1-64");
  if (obs_dim < 1 || !upkie::pipeline_sizes(P))
    return fail(UPKIE_ERR_INVALID_ARGUMENT,
                "pipeline: obs_dim must be positive and stack * (obs_dim + act_dim in the observation) at most 256 words (the policy's obs_dim)");
  if (!(dt > 0.0) || !std::isfinite(dt)) return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: dt must be positive and finite");
  if (P.lag && (!(action_lag > 0.0) || !(dt / action_lag < 0.5)))
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: low_pass_filter needs dt / action_lag < 0.5 (Nyquist-Shannon) and action_lag > 0");
  if (!params) return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: null params (upkie_pipeline_params packs them)");
  P.dt = (float)dt;
  P.alpha = P.lag ? (float)(dt / action_lag) : 0.f;
  P.seed_lo = (unsigned)(seed & 0xffffffffu);
  P.seed_hi = (unsigned)(seed >> 32);
  P.params = params;
  *out = P;
  return UPKIE_OK;
}

extern "C" int upkie_pipeline_shape_action(int32_t num_envs, int32_t obs_dim, int32_t act_dim, int32_t stack, int32_t flags, double dt,
                                           double action_lag, const float* params, uint64_t seed, const float* action, float* prev_command,
                                           uint32_t* calls, float* command, void* stream) {
  upkie::PipelineDev P;
  if (pipeline_setup(num_envs, obs_dim, act_dim, stack, flags, dt, action_lag, params, seed, &P)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!action || !prev_command || !command || (P.action_noise && !calls))
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: null argument (action, prev_command, command; calls with action noise)");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  hipLaunchKernelGGL(upkie::pipeline_shape_action_kernel, dim3((unsigned)upkie::pipeline_blocks(num_envs, P.group_act)),
                     dim3(upkie::PIPELINE_THREADS), 0, (hipStream_t)stream, P, action, prev_command, calls, command);
  return launch_status();
}

extern "C" int upkie_pipeline_observe(int32_t num_envs, int32_t obs_dim, int32_t act_dim, int32_t stack, int32_t flags, double dt,
                                      double action_lag, const float* params, uint64_t seed, const float* next_obs, const uint8_t* terminated,
                                      const uint8_t* truncated, const float* final_obs, const float* command, float* prev_command,
                                      uint32_t* calls, float* observation, float* final_observation, void* stream) {
  upkie::PipelineDev P;
  if (pipeline_setup(num_envs, obs_dim, act_dim, stack, flags, dt, action_lag, params, seed, &P)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!next_obs || !prev_command || !observation || (P.obs_noise && !calls) || (P.action_in_obs && !command))
    return fail(UPKIE_ERR_INVALID_ARGUMENT,
                "pipeline: null argument (next_obs, prev_command, observation; calls with observation noise; command when it is in the observation)");
  if (final_obs && !final_observation) return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: final_obs needs final_observation");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  hipLaunchKernelGGL(upkie::pipeline_observe_kernel<false>, dim3((unsigned)upkie::pipeline_blocks(num_envs, P.group)),
                     dim3(upkie::PIPELINE_THREADS), 0, (hipStream_t)stream, P, next_obs, terminated, truncated, final_obs, command, prev_command,
                     calls, observation, final_observation);
  return launch_status();
}

extern "C" int upkie_pipeline_reset(int32_t num_envs, int32_t obs_dim, int32_t act_dim, int32_t stack, int32_t flags, double dt,
                                    double action_lag, const float* params, uint64_t seed, const float* obs, const uint8_t* mask,
                                    float* prev_command, uint32_t* calls, float* observation, void* stream) {
  upkie::PipelineDev P;
  if (pipeline_setup(num_envs, obs_dim, act_dim, stack, flags, dt, action_lag, params, seed, &P)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!obs || !prev_command || !observation || (P.obs_noise && !calls))
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "pipeline: null argument (obs, prev_command, observation; calls with observation noise)");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  hipLaunchKernelGGL(upkie::pipeline_observe_kernel<true>, dim3((unsigned)upkie::pipeline_blocks(num_envs, P.group)),
                     dim3(upkie::PIPELINE_THREADS), 0, (hipStream_t)stream, P, obs, mask, (const uint8_t*)nullptr, (const float*)nullptr,
                     (const float*)nullptr, prev_command, calls, observation, (float*)nullptr);
  return launch_status();
}

// ============================================================ reward terms (a declarative reward, per-term episode sums)
static int check_reward_sizes(int32_t obs_dim, int32_t act_dim, int32_t num_terms) {
  if (obs_dim < 1 || obs_dim > 256 || act_dim < 1 || act_dim > 64 || num_terms < 1 || num_terms > UPKIE_REWARD_MAX_TERMS)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: obs_dim must be in 1-256, act_dim in 1-64 and num_terms in 1-16");
  return UPKIE_OK;
}

extern "C" int64_t upkie_reward_terms_params(int32_t obs_dim, int32_t act_dim, int32_t num_terms, double dt, const int32_t* shapes,
                                             const float* weights, const float* scales, const int32_t* tap_counts,
                                             const int32_t* tap_sources, const int32_t* tap_indices, const int32_t* tap_fns,
                                             const float* tap_coefs, double clip_low, double clip_high, void* params) {
  if (check_reward_sizes(obs_dim, act_dim, num_terms)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!(dt > 0.0) || !std::isfinite(dt)) return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: dt must be positive and finite");
  if (!shapes || !weights || !scales || !tap_counts || !tap_sources || !tap_indices || !tap_fns || !tap_coefs)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: null term or tap array");
  if (!(clip_low <= clip_high)) return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: the clamp needs clip_low <= clip_high (and no NaN)");
  upkie::RewardTable T{};
  T.magic = upkie::REWARD_MAGIC, T.num_terms = num_terms, T.obs_dim = obs_dim, T.act_dim = act_dim;
  T.inv_dt = (float)(1.0 / dt);
  T.clip_low = (float)clip_low, T.clip_high = (float)clip_high;
  if (!std::isfinite(T.inv_dt)) return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: 1 / dt must be a finite float32");
  int at = 0;
  for (int k = 0; k < num_terms; ++k) {
    upkie::RewardTerm& term = T.terms[k];
    term.shape = shapes[k], term.num_taps = tap_counts[k], term.weight = weights[k], term.scale = scales[k];
    if (term.shape < UPKIE_REWARD_IDENTITY || term.shape > UPKIE_REWARD_DEADBAND)
      return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: term " + std::to_string(k) + ": unknown shape");
    if (term.num_taps < 1 || term.num_taps > UPKIE_REWARD_MAX_TAPS)
      return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: term " + std::to_string(k) + ": a term has 1-8 taps");
    if (!std::isfinite(term.weight)) return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: term " + std::to_string(k) + ": the weight must be finite");
    const bool reads_scale = term.shape == UPKIE_REWARD_EXP_ABS || term.shape == UPKIE_REWARD_EXP_SQUARE || term.shape == UPKIE_REWARD_DEADBAND;
    if (reads_scale && (!(term.scale > 0.f) || !std::isfinite(term.scale)))
      return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: term " + std::to_string(k) + ": this shape needs a positive, finite scale");
    if (!reads_scale) term.scale = 1.f;
    for (int j = 0; j < term.num_taps; ++j, ++at) {
      upkie::RewardTap& tap = term.taps[j];
      tap.source = tap_sources[at], tap.index = tap_indices[at], tap.fn = tap_fns[at], tap.coef = tap_coefs[at];
      if (tap.source < UPKIE_REWARD_OBS || tap.source > UPKIE_REWARD_TERMINATED)
        return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: term " + std::to_string(k) + ": unknown tap source");
      if (tap.fn < UPKIE_REWARD_FN_ID || tap.fn > UPKIE_REWARD_FN_COS)
        return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: term " + std::to_string(k) + ": unknown tap function");
      if (!std::isfinite(tap.coef)) return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: term " + std::to_string(k) + ": tap coefficients must be finite");
      const int limit = tap.source == UPKIE_REWARD_OBS ? obs_dim : (tap.source == UPKIE_REWARD_ACTION || tap.source == UPKIE_REWARD_ACTION_RATE) ? act_dim : 0;
      if (limit == 0) tap.index = 0;
      else if (tap.index < 0 || tap.index >= limit)
        return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: term " + std::to_string(k) + ": tap index " + std::to_string(tap.index) + " is beyond the " +
                                                     (tap.source == UPKIE_REWARD_OBS ? "observation's " : "action's ") + std::to_string(limit) + " words");
    }
  }
  if (params) std::memcpy(params, &T, sizeof(T));
  return (int64_t)sizeof(T);
}

extern "C" int upkie_reward_terms_step(int32_t num_envs, int32_t obs_dim, int32_t act_dim, int32_t num_terms, const void* params,
                                       const float* next_obs, const float* action, const uint8_t* terminated, const uint8_t* truncated,
                                       const float* final_obs, float* prev_action, double* term_sum, double* term_last, int32_t* finished,
                                       float* reward, void* stream) {
  if (num_envs <= 0) return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: num_envs must be positive");
  if (check_reward_sizes(obs_dim, act_dim, num_terms)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!params || !next_obs || !action || !prev_action || !term_sum || !term_last || !finished || !reward)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: null argument (only terminated, truncated and final_obs may be NULL)");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  upkie::RewardDev P{};
  P.num_envs = num_envs, P.obs_dim = obs_dim, P.act_dim = act_dim, P.num_terms = num_terms;
  P.row16 = obs_dim == 4 && (((uintptr_t)next_obs | (uintptr_t)final_obs) & 15u) == 0;
  P.table = params, P.next_obs = next_obs, P.action = action, P.terminated = terminated, P.truncated = truncated, P.final_obs = final_obs;
  P.prev_action = prev_action, P.term_sum = term_sum, P.term_last = term_last, P.finished = finished, P.reward = reward;
  hipLaunchKernelGGL(upkie::reward_terms_step_kernel, dim3((unsigned)((num_envs + upkie::REWARD_THREADS - 1) / upkie::REWARD_THREADS)),
                     dim3(upkie::REWARD_THREADS), 0, (hipStream_t)stream, P);
  return launch_status();
}

extern "C" int upkie_reward_terms_reset(int32_t num_envs, int32_t act_dim, int32_t num_terms, const uint8_t* mask, float* prev_action,
                                        double* term_sum, void* stream) {
  if (num_envs <= 0) return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: num_envs must be positive");
  if (check_reward_sizes(1, act_dim, num_terms)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!prev_action || !term_sum) return fail(UPKIE_ERR_INVALID_ARGUMENT, "reward: null state buffer");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  hipLaunchKernelGGL(upkie::reward_terms_reset_kernel, dim3((unsigned)((num_envs + upkie::REWARD_THREADS - 1) / upkie::REWARD_THREADS)),
                     dim3(upkie::REWARD_THREADS), 0, (hipStream_t)stream, num_envs, act_dim, num_terms, mask, prev_action, term_sum);
  return launch_status();
}

// ============================================================ running normalisation (VecNormalize)
static int check_vecnorm_shape(int32_t num_envs, int32_t obs_dim) {
  if (num_envs <= 0 || obs_dim < 1 || obs_dim > 256 || (int64_t)num_envs * obs_dim > INT_MAX)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "num_envs must be positive and obs_dim in 1-256 (num_envs * obs_dim below 2^31)");
  return UPKIE_OK;
}

extern "C" int64_t upkie_vecnorm_workspace_bytes(int32_t num_envs, int32_t obs_dim) {
  if (check_vecnorm_shape(num_envs, obs_dim)) return UPKIE_ERR_INVALID_ARGUMENT;
  const int blocks = upkie::vecnorm_blocks(num_envs, obs_dim, nullptr);
  return upkie::VECNORM_PARTIALS_OFFSET + (int64_t)blocks * 2 * (obs_dim + 1) * (int64_t)sizeof(double);
}

// The launch arguments of upkie_vecnorm_step (and of its data-parallel halves) after the argument checks; returns
// UPKIE_OK or the error status. *moments / *apply: whether launch A / launch B runs.
static int vecnorm_setup(int32_t num_envs, int32_t obs_dim, const float* obs, const float* reward, const uint8_t* terminated,
                         const uint8_t* truncated, double* obs_stats, double* ret_stats, double* returns, void* workspace, int32_t flags,
                         double gamma, double epsilon, double clip_obs, double clip_reward, float* mean_f32, float* std_f32, float* packed_stats,
                         float* norm_obs, float* norm_reward, uint8_t* episode_starts, upkie::VecNormDev* out, bool* moments_out, bool* apply_out) {
  if (check_vecnorm_shape(num_envs, obs_dim)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (flags & ~(UPKIE_VECNORM_TRAINING | UPKIE_VECNORM_NORM_OBS | UPKIE_VECNORM_NORM_REWARD | UPKIE_VECNORM_RESET))
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "unknown vecnorm flags");
  if (!(gamma >= 0.0 && gamma <= 1.0) || !(epsilon > 0.0) || !(clip_obs > 0.0) || !(clip_reward > 0.0))
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "gamma must be in [0, 1], epsilon, clip_obs and clip_reward positive");
  const bool training = flags & UPKIE_VECNORM_TRAINING, reset = flags & UPKIE_VECNORM_RESET;
  upkie::VecNormDev P{};
  P.num_envs = num_envs;
  P.obs_dim = obs_dim;
  P.packed_dp = (obs_dim + 3) / 4 * 4;
  P.obs_cols = training && (flags & UPKIE_VECNORM_NORM_OBS) ? obs_dim : 0;
  P.ret_col = training && !reset ? 1 : 0;
  P.reset = reset;
  P.norm_obs = (flags & UPKIE_VECNORM_NORM_OBS) != 0;
  P.norm_reward = (flags & UPKIE_VECNORM_NORM_REWARD) != 0;
  const bool moments = P.obs_cols + P.ret_col > 0;
  const bool apply = !moments || norm_obs || (norm_reward && P.norm_reward);
  P.outputs_in_moments = moments && !apply;
  if (!obs_stats || !ret_stats || !returns || !mean_f32 || !std_f32)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "null statistics, returns or fp32 mirror buffer");
  if ((P.obs_cols || norm_obs) && !obs) return fail(UPKIE_ERR_INVALID_ARGUMENT, "updating or normalising observations needs obs");
  if ((P.ret_col || norm_reward) && !reward) return fail(UPKIE_ERR_INVALID_ARGUMENT, "updating the returns or writing norm_reward needs reward");
  if (moments && !workspace) return fail(UPKIE_ERR_INVALID_ARGUMENT, "training needs the workspace");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  P.blocks = upkie::vecnorm_blocks(num_envs, obs_dim, &P.rows);
  P.gamma = gamma, P.eps = epsilon, P.clip_obs = clip_obs, P.clip_reward = clip_reward;
  P.obs = obs, P.reward = reward, P.terminated = terminated, P.truncated = truncated;
  P.obs_stats = obs_stats, P.ret_stats = ret_stats, P.returns = returns;
  P.ticket = (unsigned*)workspace;
  P.partials = workspace ? (double*)((char*)workspace + upkie::VECNORM_PARTIALS_OFFSET) : nullptr;
  P.mean_f32 = mean_f32, P.std_f32 = std_f32, P.packed = packed_stats;
  P.norm_obs_out = norm_obs, P.reward_out = norm_reward, P.starts_out = episode_starts;
  *out = P;
  *moments_out = moments;
  *apply_out = apply;
  return UPKIE_OK;
}

static void vecnorm_launch_apply(const upkie::VecNormDev& P, hipStream_t s) {
  const int64_t work = P.norm_obs_out ? (int64_t)P.num_envs * P.obs_dim : P.num_envs;
  const int64_t grid = std::min<int64_t>((work + upkie::VECNORM_THREADS - 1) / upkie::VECNORM_THREADS, 1024);
  hipLaunchKernelGGL(upkie::vecnorm_apply_kernel, dim3((unsigned)grid), dim3(upkie::VECNORM_THREADS), 0, s, P);
}

extern "C" int upkie_vecnorm_step(int32_t num_envs, int32_t obs_dim, const float* obs, const float* reward, const uint8_t* terminated,
                                  const uint8_t* truncated, double* obs_stats, double* ret_stats, double* returns, void* workspace, int32_t flags,
                                  double gamma, double epsilon, double clip_obs, double clip_reward, float* mean_f32, float* std_f32,
                                  float* packed_stats, float* norm_obs, float* norm_reward, uint8_t* episode_starts, void* stream) {
  upkie::VecNormDev P;
  bool moments, apply;
  const int status = vecnorm_setup(num_envs, obs_dim, obs, reward, terminated, truncated, obs_stats, ret_stats, returns, workspace, flags, gamma,
                                   epsilon, clip_obs, clip_reward, mean_f32, std_f32, packed_stats, norm_obs, norm_reward, episode_starts, &P,
                                   &moments, &apply);
  if (status != UPKIE_OK) return status;
  const hipStream_t s = (hipStream_t)stream;
  if (moments) hipLaunchKernelGGL(upkie::vecnorm_moments_kernel, dim3((unsigned)P.blocks), dim3(upkie::VECNORM_THREADS), 0, s, P);
  if (apply) vecnorm_launch_apply(P, s);
  return launch_status();
}

// Whether a step with these flags moves a statistic (launch A runs): the steps of the data-parallel form.
static bool vecnorm_moves(int32_t flags) {
  return (flags & UPKIE_VECNORM_TRAINING) && ((flags & UPKIE_VECNORM_NORM_OBS) || !(flags & UPKIE_VECNORM_RESET));
}

extern "C" int64_t upkie_vecnorm_slot_bytes(int32_t obs_dim) {
  if (obs_dim < 1 || obs_dim > 256) return fail(UPKIE_ERR_INVALID_ARGUMENT, "obs_dim must be in 1-256");
  return 8 * (int64_t)upkie::vecnorm_slot_doubles(obs_dim);
}

extern "C" int upkie_vecnorm_moments_local(int32_t num_envs, int32_t obs_dim, const float* obs, const float* reward, const uint8_t* terminated,
                                           const uint8_t* truncated, double* obs_stats, double* ret_stats, double* returns, void* workspace,
                                           int32_t flags, double gamma, double epsilon, double clip_obs, double clip_reward, float* mean_f32,
                                           float* std_f32, float* packed_stats, float* norm_obs, float* norm_reward, uint8_t* episode_starts,
                                           double* slot, void* stream) {
  if (!vecnorm_moves(flags) || !slot)
    return fail(UPKIE_ERR_INVALID_ARGUMENT,
                "upkie_vecnorm_moments_local needs a step that moves a statistic (TRAINING, and NORM_OBS or not RESET) and a slot");
  upkie::VecNormDev P;
  bool moments, apply;
  const int status = vecnorm_setup(num_envs, obs_dim, obs, reward, terminated, truncated, obs_stats, ret_stats, returns, workspace, flags, gamma,
                                   epsilon, clip_obs, clip_reward, mean_f32, std_f32, packed_stats, norm_obs, norm_reward, episode_starts, &P,
                                   &moments, &apply);
  if (status != UPKIE_OK) return status;
  P.slot = slot;
  hipLaunchKernelGGL(upkie::vecnorm_moments_kernel, dim3((unsigned)P.blocks), dim3(upkie::VECNORM_THREADS), 0, (hipStream_t)stream, P);
  return launch_status();
}

extern "C" int upkie_vecnorm_merge(int32_t num_envs, int32_t obs_dim, const float* obs, const float* reward, const uint8_t* terminated,
                                   const uint8_t* truncated, double* obs_stats, double* ret_stats, double* returns, void* workspace, int32_t flags,
                                   double gamma, double epsilon, double clip_obs, double clip_reward, float* mean_f32, float* std_f32,
                                   float* packed_stats, float* norm_obs, float* norm_reward, uint8_t* episode_starts, const double* slots,
                                   int32_t world, void* stream) {
  if (!vecnorm_moves(flags) || !slots || world < 1)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "upkie_vecnorm_merge needs a step that moves a statistic, the exchanged slots and world >= 1");
  upkie::VecNormDev P;
  bool moments, apply;
  const int status = vecnorm_setup(num_envs, obs_dim, obs, reward, terminated, truncated, obs_stats, ret_stats, returns, workspace, flags, gamma,
                                   epsilon, clip_obs, clip_reward, mean_f32, std_f32, packed_stats, norm_obs, norm_reward, episode_starts, &P,
                                   &moments, &apply);
  if (status != UPKIE_OK) return status;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(upkie::vecnorm_merge_kernel, dim3(1), dim3(upkie::VECNORM_THREADS), 0, s, P, slots, (int)world,
                     upkie::vecnorm_slot_doubles(obs_dim));
  if (apply) vecnorm_launch_apply(P, s);
  return launch_status();
}

// ============================================================ rollout consumer
extern "C" int upkie_linear_policy(int32_t num_envs, int32_t obs_dim, int32_t act_dim, const float* obs, const float* weights, const float* bias,
                                  double clip, float* act, void* stream) {
  if (num_envs <= 0 || obs_dim <= 0 || act_dim <= 0) return fail(UPKIE_ERR_INVALID_ARGUMENT, "num_envs, obs_dim and act_dim must be positive");
  if (!obs || !weights || !act) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  hipLaunchKernelGGL(upkie::linear_policy_kernel, dim3((unsigned)((num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, num_envs, obs_dim,
                     act_dim, obs, weights, bias, (float)clip, act);
  return launch_status();
}

extern "C" int upkie_rollout_gae(int32_t num_steps, int32_t num_envs, const float* rewards, const float* values,
                                 const uint8_t* episode_starts, const float* last_values, const uint8_t* last_dones, double gamma,
                                 double gae_lambda, float* advantages, float* returns, void* stream) {
  if (num_steps <= 0 || num_envs <= 0) return fail(UPKIE_ERR_INVALID_ARGUMENT, "num_steps and num_envs must be positive");
  if (!rewards || !values || !episode_starts || !last_values || !last_dones || !advantages || !returns)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  hipLaunchKernelGGL(upkie::gae_kernel, dim3((unsigned)((num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, num_steps, num_envs,
                     rewards, values, episode_starts, last_values, last_dones, (float)gamma, (float)gae_lambda, advantages, returns);
  return launch_status();
}

// ============================================================ privileged observation (the asymmetric critic's row)
extern "C" int upkie_privileged_observation(int32_t num_envs, int32_t obs_dim, int32_t act_dim, int32_t num_segments, const int32_t* kinds,
                                            const int32_t* counts, const float* next_obs, const float* final_obs, const float* command,
                                            const float* force, const float* link_scale, const int32_t* links, const uint8_t* terminated,
                                            const uint8_t* truncated, int32_t reset, float* observation, float* final_observation,
                                            void* stream) {
  if (num_envs <= 0 || obs_dim < 1 || obs_dim > 256 || act_dim < 1 || act_dim > 64)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "privileged: num_envs must be positive, obs_dim in 1-256 and act_dim in 1-64");
  if (!kinds || !counts) return fail(UPKIE_ERR_INVALID_ARGUMENT, "privileged: null segment arrays");
  upkie::PrivilegedDev P{};
  P.num_envs = num_envs, P.obs_dim = obs_dim, P.act_dim = act_dim, P.num_segments = num_segments, P.reset = reset ? 1 : 0;
  for (int k = 0; k < num_segments && k < UPKIE_PRIVILEGED_MAX_SEGMENTS; ++k) P.kind[k] = kinds[k], P.count[k] = counts[k];
  if (!upkie::privileged_layout(P))
    return fail(UPKIE_ERR_INVALID_ARGUMENT,
                "privileged: 1-8 segments of a known kind; observation words at most obs_dim, command words at most act_dim, 1-3 force words, "
                "1-24 link scales; a row of at most 256 words, at most 32 of them force or scale words");
  if ((int64_t)num_envs * P.row_dim > INT_MAX) return fail(UPKIE_ERR_INVALID_ARGUMENT, "privileged: num_envs * row_dim must stay below 2^31");
  for (int k = 0; k < num_segments; ++k) {
    const void* source = P.kind[k] == UPKIE_PRIVILEGED_OBSERVATION ? (const void*)next_obs
                         : P.kind[k] == UPKIE_PRIVILEGED_COMMAND   ? (const void*)command
                         : P.kind[k] == UPKIE_PRIVILEGED_PUSH_FORCE ? (const void*)force
                                                                    : (const void*)link_scale;
    if (!source || (P.kind[k] == UPKIE_PRIVILEGED_LINK_SCALE && !links))
      return fail(UPKIE_ERR_INVALID_ARGUMENT, "privileged: segment " + std::to_string(k) + " has no source buffer (link scales also need links)");
  }
  if (!observation || (!P.reset && !final_observation))
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "privileged: null observation (or final_observation outside a reset)");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  P.next_obs = next_obs, P.final_obs = final_obs, P.command = command, P.force = force, P.link_scale = link_scale, P.links = links;
  P.terminated = terminated, P.truncated = truncated, P.observation = observation, P.final_observation = final_observation;
  const unsigned blocks = (unsigned)((num_envs + upkie::PRIVILEGED_ENVS - 1) / upkie::PRIVILEGED_ENVS);
  hipLaunchKernelGGL(upkie::privileged_observation_kernel, dim3(blocks), dim3(upkie::PRIVILEGED_THREADS), 0, (hipStream_t)stream, P);
  return launch_status();
}
