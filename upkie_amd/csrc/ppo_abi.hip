// ppo_abi.hip -- the PPO update of include/upkie_hip.h (one rank, data-parallel and controlled forms): host code around
// the kernels of ppo.hpp, and the distillation update (distill.hpp), whose launches are ppo.hpp's kernels under another head
// and so live in the unit that defines them. Handle-free like trainer_abi.hip, and a unit of its own because its gradient-
// kernel instantiations (ten of PPO, ten of its mirrored form, ten of the behaviour-cloning head) take as long to compile as everything else outside
// the step kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "distill.hpp"
#include "mlp_instances.hpp"
#include "ppo.hpp"

#include "abi_host.hpp"

static int check_ppo_shape(const UpkieMlpShape* shape, upkie::PpoPlan* plan) {
  if (!shape) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null shape");
  if (upkie::mlp_layout(*shape, nullptr) < 0) return (int)upkie_mlp_packed_words(shape);  // (sets the message)
  if (!upkie::ppo_plan(*shape, plan)) return fail(UPKIE_ERR_INVALID_ARGUMENT, "PPO needs a critic (critic_layers > 0)");
  return UPKIE_OK;
}

extern "C" int64_t upkie_ppo_workspace_bytes(const UpkieMlpShape* shape, int32_t max_minibatch) {
  upkie::PpoPlan plan;
  if (check_ppo_shape(shape, &plan)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (max_minibatch < 1) return fail(UPKIE_ERR_INVALID_ARGUMENT, "max_minibatch must be positive");
  return upkie::ppo_workspace_bytes(plan, upkie::ppo_grid(plan, max_minibatch));
}

extern "C" int upkie_ppo_advantage_stats(int32_t total, int32_t batch_size, const int32_t* perm, const float* advantages, int32_t normalize,
                                         double* adv_stats, void* stream) {
  if (total < 1 || batch_size < 1) return fail(UPKIE_ERR_INVALID_ARGUMENT, "total and batch_size must be positive");
  if (!perm || !advantages || !adv_stats) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  const unsigned blocks = (unsigned)((total + (int64_t)batch_size - 1) / batch_size);
  hipLaunchKernelGGL(upkie::ppo_adv_stats_kernel, dim3(blocks), dim3(upkie::PPO_ADV_THREADS), 0, (hipStream_t)stream, total, batch_size, perm,
                     advantages, normalize ? 1 : 0, adv_stats);
  return launch_status();
}

static int check_ppo_config(const UpkiePpoConfig* config) {
  if (!config) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null config");
  const UpkiePpoConfig& c = *config;
  if (!(c.clip_range > 0.f) || !(c.max_grad_norm > 0.f) || !(c.adam_eps > 0.f) || !(c.adam_beta1 >= 0.f && c.adam_beta1 < 1.f) ||
      !(c.adam_beta2 >= 0.f && c.adam_beta2 < 1.f) || !std::isfinite(c.ent_coef) || !std::isfinite(c.vf_coef) ||
      !(c.clip_range_vf == c.clip_range_vf))
    return fail(UPKIE_ERR_INVALID_ARGUMENT,
                "config: clip_range, max_grad_norm and adam_eps must be positive, adam betas in [0, 1), coefficients finite");
  return UPKIE_OK;
}

// The fields of every launch of a minibatch but the gradient launch's inputs, and the workspace layout for minibatches
// of at most max_minibatch samples.
static void ppo_fill(upkie::PpoDev& P, const UpkieMlpShape& shape, const upkie::PpoPlan& plan, const UpkiePpoConfig& c, int max_minibatch,
                     void* workspace) {
  upkie::mlp_layout(shape, &P.net);
  P.stage[0] = plan.stage[0], P.stage[1] = plan.stage[1];
  P.train_off = plan.train_off, P.train_words = plan.train_words;
  P.nw = plan.nw, P.tile_floats = plan.tile_floats;
  const int ws_grid = upkie::ppo_grid(plan, max_minibatch);  // (the workspace's layout)
  P.fold_blocks = plan.fold_blocks;
  P.part_stride = plan.train_words, P.stat_stride = upkie::PPO_STATS;
  P.obs_normalized = c.obs_normalized ? 1 : 0;
  P.vf_clip = c.clip_range_vf > 0.f;
  P.clip_range = c.clip_range;
  P.clip_lo = (float)(1.0 - (double)c.clip_range), P.clip_hi = (float)(1.0 + (double)c.clip_range);
  P.clip_vf = c.clip_range_vf, P.ent_coef = c.ent_coef, P.vf_coef = c.vf_coef, P.max_grad_norm = c.max_grad_norm;
  P.beta1 = c.adam_beta1, P.beta2 = c.adam_beta2, P.adam_eps = c.adam_eps;
  char* ws = (char*)workspace;
  P.ticket = (unsigned*)ws;
  P.header = (float*)ws;
  P.partials = (float*)(ws + upkie::PPO_HEADER_BYTES);
  P.stat_partials = (double*)(ws + upkie::ppo_stat_partials_at(plan, ws_grid));
  P.grad = (float*)(ws + upkie::ppo_grad_at(plan, ws_grid));
  P.sq_partials = (double*)(ws + upkie::ppo_sq_at(plan, ws_grid));
}

// Checks and fields of the gradient launch (launch A) of minibatch [minibatch_start, + minibatch_size).
static int ppo_gradient_setup(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total, int32_t minibatch_start,
                              int32_t minibatch_size, int32_t count, int32_t max_minibatch, const int32_t* perm, const float* obs,
                              const float* critic_obs, const float* actions, const float* old_values, const float* old_log_prob, const float* advantages,
                              const float* returns, const double* adv_stats, float* packed, void* workspace, upkie::PpoDev* out,
                              upkie::PpoPlan* plan) {
  if (check_ppo_shape(shape, plan)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!critic_obs && shape->critic_obs_dim != 0)  // (the entry points without critic_obs hand NULL down)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "the shape is asymmetric (critic_obs_dim " + std::to_string(shape->critic_obs_dim) + ", obs_dim " +
                                                std::to_string(shape->obs_dim) +
                                                "): the critic's rows go to upkie_ppo_minibatch_update_asym / upkie_ppo_minibatch_gradient_asym");
  if (check_ppo_config(config)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (total < 1 || minibatch_size < 1 || max_minibatch < 1 || minibatch_start < 0 || minibatch_size > max_minibatch ||
      (int64_t)minibatch_start + minibatch_size > total || count < minibatch_size)
    return fail(UPKIE_ERR_INVALID_ARGUMENT,
                "minibatch out of range: 0 <= minibatch_start, 1 <= minibatch_size <= max_minibatch, start + size <= total, global size >= size");
  if ((int64_t)total * std::max(std::max(shape->obs_dim, shape->act_dim), shape->critic_obs_dim) > INT_MAX)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "total * obs_dim (or act_dim, or critic_obs_dim) must stay below 2^31");
  if (!perm || !obs || !actions || !old_values || !old_log_prob || !advantages || !returns || !adv_stats || !packed || !workspace)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  upkie::PpoDev P{};
  ppo_fill(P, *shape, *plan, *config, max_minibatch, workspace);
  P.mb_start = minibatch_start, P.mb_size = minibatch_size, P.count = count;
  P.grid = upkie::ppo_grid(*plan, minibatch_size);
  P.asym = shape->critic_obs_dim != 0;
  P.perm = perm, P.obs = obs, P.critic_obs = P.asym ? critic_obs : obs, P.actions = actions, P.old_values = old_values, P.old_log_prob = old_log_prob;
  P.advantages = advantages, P.returns = returns, P.adv_stats = adv_stats;
  P.packed = packed;
  *out = P;
  return UPKIE_OK;
}

// The gradient launch (launch A) of a minibatch, and its status. MIR: the mirrored form's instantiation.
template <bool MIR = false>
static int ppo_launch_gradient(const UpkieMlpShape& shape, const upkie::PpoDev& P, const upkie::PpoPlan& plan, hipStream_t s) {
  return for_mlp_instance(shape, [&](auto w, auto act) {
    auto kernel = upkie::ppo_grad_kernel<w(), act(), false, MIR>;
    if (plan.lds_bytes > upkie::PPO_LDS_BUDGET) {
      // (one tile of the widest shapes needs more than 64 KiB; MI355X has 160 KiB per CU). Raised once per instantiation, to
      // what any valid shape of it can need, so that a later shape with a larger stage is covered too: `raised` is a static
      // of this generic lambda's call operator, which for_mlp_instance instantiates once per (width class, activation).
      static const hipError_t raised = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, upkie::PPO_LDS_MAX);
      if (raised != hipSuccess) return launch_status(raised);
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)P.grid), dim3(64 * P.nw), (size_t)plan.lds_bytes, s, P);
    return launch_status();
  });
}

// A control block: PPO_CTRL_WORDS doubles in device memory.
static int check_ppo_control(const double* control) {
  if (!control) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null control block");
  if ((uintptr_t)control % 8 != 0) return fail(UPKIE_ERR_INVALID_ARGUMENT, "the control block must be 8-byte aligned");
  return UPKIE_OK;
}

// upkie_ppo_minibatch_update (control == nullptr) and upkie_ppo_minibatch_update_controlled.
static int ppo_minibatch_update(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total, int32_t minibatch_start,
                                int32_t minibatch_size, int32_t max_minibatch, const int32_t* perm, const float* obs, const float* critic_obs,
                                const float* actions, const float* old_values, const float* old_log_prob, const float* advantages, const float* returns,
                                const double* adv_stats, float* packed, float* adam_m, float* adam_v, double* adam_scalars, double* control,
                                void* workspace, float* stats, void* stream) {
  upkie::PpoPlan plan;
  upkie::PpoDev P;
  if (!adam_m || !adam_v || !adam_scalars || !stats) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument");
  int status = ppo_gradient_setup(shape, config, total, minibatch_start, minibatch_size, minibatch_size, max_minibatch, perm, obs, critic_obs, actions,
                                  old_values, old_log_prob, advantages, returns, adv_stats, packed, workspace, &P, &plan);
  if (status != UPKIE_OK) return status;
  P.m = adam_m, P.v = adam_v, P.scalars = adam_scalars, P.ctrl = control, P.stats = stats;
  const hipStream_t s = (hipStream_t)stream;
  status = ppo_launch_gradient(*shape, P, plan, s);
  if (status != UPKIE_OK) return status;
  hipLaunchKernelGGL(upkie::ppo_fold_kernel, dim3((unsigned)P.fold_blocks), dim3(upkie::PPO_THREADS), 0, s, P);
  hipLaunchKernelGGL(upkie::ppo_adam_kernel, dim3((unsigned)P.fold_blocks), dim3(upkie::PPO_THREADS), 0, s, P);
  return launch_status();
}

extern "C" int upkie_ppo_minibatch_update(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total, int32_t minibatch_start,
                                          int32_t minibatch_size, int32_t max_minibatch, const int32_t* perm, const float* obs,
                                          const float* actions, const float* old_values, const float* old_log_prob, const float* advantages,
                                          const float* returns, const double* adv_stats, float* packed, float* adam_m, float* adam_v,
                                          double* adam_scalars, void* workspace, float* stats, void* stream) {
  return ppo_minibatch_update(shape, config, total, minibatch_start, minibatch_size, max_minibatch, perm, obs, nullptr, actions, old_values, old_log_prob,
                              advantages, returns, adv_stats, packed, adam_m, adam_v, adam_scalars, nullptr, workspace, stats, stream);
}

// ---- controlled form (a control block instead of adam_scalars; include/upkie_hip.h)
extern "C" int upkie_ppo_minibatch_update_controlled(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total,
                                                     int32_t minibatch_start, int32_t minibatch_size, int32_t max_minibatch, const int32_t* perm,
                                                     const float* obs, const float* actions, const float* old_values, const float* old_log_prob,
                                                     const float* advantages, const float* returns, const double* adv_stats, float* packed,
                                                     float* adam_m, float* adam_v, double* control, void* workspace, float* stats, void* stream) {
  if (check_ppo_control(control)) return UPKIE_ERR_INVALID_ARGUMENT;
  return ppo_minibatch_update(shape, config, total, minibatch_start, minibatch_size, max_minibatch, perm, obs, nullptr, actions, old_values, old_log_prob,
                              advantages, returns, adv_stats, packed, adam_m, adam_v, control, control, workspace, stats, stream);
}

extern "C" int upkie_ppo_control_set(double* control, double lr, double clip_range, double clip_range_vf, double target_kl, void* stream) {
  if (check_ppo_control(control)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!(lr >= 0.0) || !std::isfinite(lr) || !(clip_range > 0.0) || !std::isfinite(clip_range) || !(clip_range_vf >= 0.0) ||
      !std::isfinite(clip_range_vf) || !(target_kl >= 0.0) || !std::isfinite(target_kl))
    return fail(UPKIE_ERR_INVALID_ARGUMENT,
                "control: lr, clip_range_vf (0: none) and target_kl (0: none) must be finite and not negative, clip_range positive");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  hipLaunchKernelGGL(upkie::ppo_control_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, control, lr, clip_range, clip_range_vf, target_kl);
  return launch_status();
}

extern "C" int upkie_ppo_update_begin(double* control, void* stream) {
  if (check_ppo_control(control)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  hipLaunchKernelGGL(upkie::ppo_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, control);
  return launch_status();
}

extern "C" int upkie_ppo_explained_variance(int32_t total, const float* returns, const float* values, int32_t phase, const double* slots,
                                            int32_t world, double* slot, double* out, void* stream) {
  if (total < 1 || phase < -1 || phase > 2 || (phase >= 0 && world < 1))
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "total and world must be positive, phase -1 (one rank), 0, 1 or 2");
  if (((phase < 0 || phase == 0 || phase == 1) && (!returns || !values)) || ((phase == 0 || phase == 1) && !slot) || (phase >= 1 && !slots) ||
      ((phase < 0 || phase == 2) && !out))
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  hipLaunchKernelGGL(upkie::ppo_explained_variance_kernel, dim3(1), dim3(upkie::PPO_ADV_THREADS), 0, (hipStream_t)stream, (int)total, returns,
                     values, (int)phase, slots, (int)world, slot, out);
  return launch_status();
}

// ---- data-parallel form (several ranks; include/upkie_hip.h)
extern "C" int64_t upkie_ppo_slot_bytes(const UpkieMlpShape* shape) {
  upkie::PpoPlan plan;
  if (check_ppo_shape(shape, &plan)) return UPKIE_ERR_INVALID_ARGUMENT;
  return 4 * (int64_t)upkie::ppo_slot_words(plan);
}

static int ppo_minibatch_gradient(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total, int32_t minibatch_start,
                                  int32_t minibatch_size, int32_t global_minibatch_size, int32_t max_minibatch, const int32_t* perm,
                                  const float* obs, const float* critic_obs, const float* actions, const float* old_values, const float* old_log_prob,
                                  const float* advantages, const float* returns, const double* adv_stats, float* packed, void* workspace,
                                  void* slot, double* control, void* stream) {
  upkie::PpoPlan plan;
  upkie::PpoDev P;
  if (!slot) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null slot");
  int status = ppo_gradient_setup(shape, config, total, minibatch_start, minibatch_size, global_minibatch_size, max_minibatch, perm, obs, critic_obs, actions,
                                  old_values, old_log_prob, advantages, returns, adv_stats, packed, workspace, &P, &plan);
  if (status != UPKIE_OK) return status;
  P.slot = (float*)slot;
  P.ctrl = control;
  const hipStream_t s = (hipStream_t)stream;
  status = ppo_launch_gradient(*shape, P, plan, s);
  if (status != UPKIE_OK) return status;
  hipLaunchKernelGGL(upkie::ppo_local_fold_kernel, dim3((unsigned)P.fold_blocks), dim3(upkie::PPO_THREADS), 0, s, P);
  return launch_status();
}

extern "C" int upkie_ppo_minibatch_gradient(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total, int32_t minibatch_start,
                                            int32_t minibatch_size, int32_t global_minibatch_size, int32_t max_minibatch, const int32_t* perm,
                                            const float* obs, const float* actions, const float* old_values, const float* old_log_prob,
                                            const float* advantages, const float* returns, const double* adv_stats, float* packed, void* workspace,
                                            void* slot, void* stream) {
  return ppo_minibatch_gradient(shape, config, total, minibatch_start, minibatch_size, global_minibatch_size, max_minibatch, perm, obs, nullptr, actions,
                                old_values, old_log_prob, advantages, returns, adv_stats, packed, workspace, slot, nullptr, stream);
}

extern "C" int upkie_ppo_minibatch_gradient_controlled(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total,
                                                       int32_t minibatch_start, int32_t minibatch_size, int32_t global_minibatch_size,
                                                       int32_t max_minibatch, const int32_t* perm, const float* obs, const float* actions,
                                                       const float* old_values, const float* old_log_prob, const float* advantages,
                                                       const float* returns, const double* adv_stats, float* packed, void* workspace, void* slot,
                                                       double* control, void* stream) {
  if (check_ppo_control(control)) return UPKIE_ERR_INVALID_ARGUMENT;
  return ppo_minibatch_gradient(shape, config, total, minibatch_start, minibatch_size, global_minibatch_size, max_minibatch, perm, obs, nullptr, actions,
                                old_values, old_log_prob, advantages, returns, adv_stats, packed, workspace, slot, control, stream);
}

// ---- asymmetric shapes: the critic's rows beside obs, a nullable control block (include/upkie_hip.h)
extern "C" int upkie_ppo_minibatch_update_asym(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total, int32_t minibatch_start,
                                               int32_t minibatch_size, int32_t max_minibatch, const int32_t* perm, const float* obs,
                                               const float* critic_obs, const float* actions, const float* old_values, const float* old_log_prob,
                                               const float* advantages, const float* returns, const double* adv_stats, float* packed,
                                               float* adam_m, float* adam_v, double* adam_scalars, double* control, void* workspace, float* stats,
                                               void* stream) {
  if (!critic_obs) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null critic_obs");
  if (control && check_ppo_control(control)) return UPKIE_ERR_INVALID_ARGUMENT;
  return ppo_minibatch_update(shape, config, total, minibatch_start, minibatch_size, max_minibatch, perm, obs, critic_obs, actions, old_values,
                              old_log_prob, advantages, returns, adv_stats, packed, adam_m, adam_v, control ? control : adam_scalars, control,
                              workspace, stats, stream);
}

extern "C" int upkie_ppo_minibatch_gradient_asym(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t total, int32_t minibatch_start,
                                                 int32_t minibatch_size, int32_t global_minibatch_size, int32_t max_minibatch,
                                                 const int32_t* perm, const float* obs, const float* critic_obs, const float* actions,
                                                 const float* old_values, const float* old_log_prob, const float* advantages,
                                                 const float* returns, const double* adv_stats, float* packed, void* workspace, void* slot,
                                                 double* control, void* stream) {
  if (!critic_obs) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null critic_obs");
  if (control && check_ppo_control(control)) return UPKIE_ERR_INVALID_ARGUMENT;
  return ppo_minibatch_gradient(shape, config, total, minibatch_start, minibatch_size, global_minibatch_size, max_minibatch, perm, obs,
                                critic_obs, actions, old_values, old_log_prob, advantages, returns, adv_stats, packed, workspace, slot, control,
                                stream);
}

// ---- the mirrored form: augmented samples and the mirror loss (include/upkie_hip.h)
extern "C" int64_t upkie_ppo_mirror_words(const UpkieMlpShape* shape) {
  upkie::PpoPlan plan;
  if (check_ppo_shape(shape, &plan)) return UPKIE_ERR_INVALID_ARGUMENT;
  return upkie::ppo_mirror_words(*shape);
}

// One table of a mirror: every index in range, every sign +1 or -1, index an involution whose partners carry equal signs.
static int check_mirror_table(const char* name, int dim, const int32_t* index, const float* sign) {
  const std::string what = std::string("mirror: ") + name;
  for (int k = 0; k < dim; ++k) {
    if (index[k] < 0 || index[k] >= dim)
      return fail(UPKIE_ERR_INVALID_ARGUMENT, what + "_index[" + std::to_string(k) + "] = " + std::to_string(index[k]) + " is out of range [0, " +
                                                  std::to_string(dim) + ")");
    if (!(sign[k] == 1.f || sign[k] == -1.f))
      return fail(UPKIE_ERR_INVALID_ARGUMENT, what + "_sign[" + std::to_string(k) + "] must be +1 or -1");
  }
  for (int k = 0; k < dim; ++k) {
    if (index[index[k]] != k)
      return fail(UPKIE_ERR_INVALID_ARGUMENT, what + "_index is not an involution: index[index[" + std::to_string(k) + "]] != " + std::to_string(k));
    if (sign[index[k]] != sign[k])
      return fail(UPKIE_ERR_INVALID_ARGUMENT,
                  what + "_sign differs between the partners " + std::to_string(k) + " and " + std::to_string(index[k]) + " (the mirror would not be an involution)");
  }
  return UPKIE_OK;
}

extern "C" int upkie_ppo_mirror_set(const UpkieMlpShape* shape, const int32_t* obs_index, const float* obs_sign, const int32_t* critic_index,
                                    const float* critic_sign, const int32_t* act_index, const float* act_sign, void* tables, void* stream) {
  upkie::PpoPlan plan;
  if (check_ppo_shape(shape, &plan)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!obs_index || !obs_sign || !act_index || !act_sign || !tables) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument");
  const int D = shape->obs_dim, Dc = shape->critic_obs_dim, A = shape->act_dim;
  if (Dc != 0 && (!critic_index || !critic_sign))
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "mirror: the shape is asymmetric (critic_obs_dim " + std::to_string(Dc) +
                                                "): the critic's row needs critic_index and critic_sign of its own");
  if (Dc == 0 && (critic_index || critic_sign))
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "mirror: the shape is symmetric (critic_obs_dim 0): the critic reads the observation, critic tables are superfluous");
  if (check_mirror_table("obs", D, obs_index, obs_sign) || (Dc && check_mirror_table("critic", Dc, critic_index, critic_sign)) ||
      check_mirror_table("act", A, act_index, act_sign))
    return UPKIE_ERR_INVALID_ARGUMENT;
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  // the device block: index then sign of the observation, of the critic's row, of the action (ppo_mirror_words words)
  std::vector<uint32_t> block((size_t)upkie::ppo_mirror_words(*shape));
  size_t at = 0;
  auto put = [&](int dim, const int32_t* index, const float* sign) {
    if (dim == 0) return;
    std::memcpy(block.data() + at, index, 4 * (size_t)dim), at += dim;
    std::memcpy(block.data() + at, sign, 4 * (size_t)dim), at += dim;
  };
  put(D, obs_index, obs_sign), put(Dc, critic_index, critic_sign), put(A, act_index, act_sign);
  const hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipMemcpyAsync(tables, block.data(), 4 * block.size(), hipMemcpyHostToDevice, s);
  if (err == hipSuccess) err = hipStreamSynchronize(s);  // (`block` ends with this call)
  return launch_status(err);
}

extern "C" int64_t upkie_ppo_mirror_workspace_bytes(const UpkieMlpShape* shape, int32_t max_minibatch) {
  upkie::PpoPlan plan;
  if (check_ppo_shape(shape, &plan)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (max_minibatch < 1 || max_minibatch > INT_MAX / 2) return fail(UPKIE_ERR_INVALID_ARGUMENT, "max_minibatch must be positive and at most 2^30 - 1");
  return upkie::ppo_mirror_workspace_bytes(plan, upkie::ppo_mirror_grid(plan, max_minibatch));
}

extern "C" int upkie_ppo_minibatch_update_mirror(const UpkieMlpShape* shape, const UpkiePpoConfig* config, const UpkiePpoMirror* mirror, int32_t total,
                                                 int32_t minibatch_start, int32_t minibatch_size, int32_t max_minibatch, const int32_t* perm,
                                                 const float* obs, const float* critic_obs, const float* actions, const float* old_values,
                                                 const float* old_log_prob, const float* advantages, const float* returns, const double* adv_stats,
                                                 float* packed, float* adam_m, float* adam_v, double* adam_scalars, double* control, void* workspace,
                                                 float* stats, void* stream) {
  upkie::PpoPlan plan;
  upkie::PpoDev P;
  if (!mirror || !mirror->tables) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null mirror (or mirror->tables)");
  if (!(mirror->mirror_coef >= 0.f) || !std::isfinite(mirror->mirror_coef))
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "mirror: mirror_coef must be finite and not negative");
  if (max_minibatch > INT_MAX / 2) return fail(UPKIE_ERR_INVALID_ARGUMENT, "mirror: max_minibatch must be at most 2^30 - 1");
  if (control && check_ppo_control(control)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!adam_m || !adam_v || !adam_scalars || !stats) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument");
  int status = ppo_gradient_setup(shape, config, total, minibatch_start, minibatch_size, minibatch_size, max_minibatch, perm, obs, critic_obs, actions,
                                  old_values, old_log_prob, advantages, returns, adv_stats, packed, workspace, &P, &plan);
  if (status != UPKIE_OK) return status;
  P.m = adam_m, P.v = adam_v, P.scalars = control ? control : adam_scalars, P.ctrl = control, P.stats = stats;
  // the mirrored grid (2 B positions) and workspace layout (PPO_MIRROR_STATS sums per block)
  const int ws_grid = upkie::ppo_mirror_grid(plan, max_minibatch);
  char* ws = (char*)workspace;
  P.grid = upkie::ppo_mirror_grid(plan, minibatch_size);
  P.stat_stride = upkie::PPO_MIRROR_STATS;
  P.stat_partials = (double*)(ws + upkie::ppo_stat_partials_at(plan, ws_grid));
  P.grad = (float*)(ws + upkie::ppo_mirror_grad_at(plan, ws_grid));
  P.sq_partials = (double*)(ws + upkie::ppo_mirror_sq_at(plan, ws_grid));
  P.mir_augment = mirror->augment ? 1 : 0, P.mirror_coef = mirror->mirror_coef;
  const int D = shape->obs_dim, Dc = shape->critic_obs_dim, A = shape->act_dim;
  const int32_t* t = (const int32_t*)mirror->tables;
  P.mir_obs_index = t, P.mir_obs_sign = (const float*)(t + D), t += 2 * D;
  P.mir_critic_index = Dc ? t : P.mir_obs_index, P.mir_critic_sign = Dc ? (const float*)(t + Dc) : P.mir_obs_sign, t += 2 * Dc;
  P.mir_act_index = t, P.mir_act_sign = (const float*)(t + A);
  const hipStream_t s = (hipStream_t)stream;
  status = ppo_launch_gradient<true>(*shape, P, plan, s);
  if (status != UPKIE_OK) return status;
  hipLaunchKernelGGL(upkie::ppo_mirror_fold_kernel, dim3((unsigned)P.fold_blocks), dim3(upkie::PPO_THREADS), 0, s, P);
  hipLaunchKernelGGL(upkie::ppo_adam_kernel, dim3((unsigned)P.fold_blocks), dim3(upkie::PPO_THREADS), 0, s, P);
  return launch_status();
}

static int ppo_minibatch_apply(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t minibatch_start, int32_t global_minibatch_size,
                               int32_t max_minibatch, const void* slots, int32_t world, float* packed, float* adam_m, float* adam_v,
                               double* adam_scalars, double* control, void* workspace, float* stats, void* stream) {
  upkie::PpoPlan plan;
  if (check_ppo_shape(shape, &plan)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (check_ppo_config(config)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (global_minibatch_size < 1 || max_minibatch < 1 || world < 1 || minibatch_start < 0)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "global_minibatch_size, max_minibatch and world must be positive, minibatch_start not negative");
  if (!slots || !packed || !adam_m || !adam_v || !adam_scalars || !workspace || !stats) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  upkie::PpoDev P{};
  ppo_fill(P, *shape, plan, *config, max_minibatch, workspace);
  P.count = global_minibatch_size;
  P.mb_start = minibatch_start, P.ctrl = control;
  P.grid = world;  // (launch B's partials: the slots, in rank order)
  const int words = upkie::ppo_slot_words(plan);
  P.partials = (float*)slots;
  P.part_stride = words;
  P.stat_partials = (double*)((float*)slots + upkie::ppo_slot_stats_at(plan));
  P.stat_stride = words / 2;
  P.packed = packed, P.m = adam_m, P.v = adam_v, P.scalars = adam_scalars, P.stats = stats;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(upkie::ppo_fold_kernel, dim3((unsigned)P.fold_blocks), dim3(upkie::PPO_THREADS), 0, s, P);
  hipLaunchKernelGGL(upkie::ppo_adam_kernel, dim3((unsigned)P.fold_blocks), dim3(upkie::PPO_THREADS), 0, s, P);
  return launch_status();
}

extern "C" int upkie_ppo_minibatch_apply(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t global_minibatch_size,
                                         int32_t max_minibatch, const void* slots, int32_t world, float* packed, float* adam_m, float* adam_v,
                                         double* adam_scalars, void* workspace, float* stats, void* stream) {
  return ppo_minibatch_apply(shape, config, 0, global_minibatch_size, max_minibatch, slots, world, packed, adam_m, adam_v, adam_scalars, nullptr,
                             workspace, stats, stream);
}

extern "C" int upkie_ppo_minibatch_apply_controlled(const UpkieMlpShape* shape, const UpkiePpoConfig* config, int32_t minibatch_start,
                                                    int32_t global_minibatch_size, int32_t max_minibatch, const void* slots, int32_t world,
                                                    float* packed, float* adam_m, float* adam_v, double* control, void* workspace, float* stats,
                                                    void* stream) {
  if (check_ppo_control(control)) return UPKIE_ERR_INVALID_ARGUMENT;
  return ppo_minibatch_apply(shape, config, minibatch_start, global_minibatch_size, max_minibatch, slots, world, packed, adam_m, adam_v, control,
                             control, workspace, stats, stream);
}

extern "C" int64_t upkie_ppo_advantage_slot_bytes(int32_t total, int32_t batch_size) {
  if (total < 1 || batch_size < 1) return fail(UPKIE_ERR_INVALID_ARGUMENT, "total and batch_size must be positive");
  return 16 * ((total + (int64_t)batch_size - 1) / batch_size);
}

extern "C" int upkie_ppo_advantage_partials(int32_t total, int32_t batch_size, const int32_t* perm, const float* advantages, int32_t phase,
                                            const double* slots, int32_t world, double* slot, void* stream) {
  if (total < 1 || batch_size < 1 || (phase != 0 && phase != 1) || world < 1)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "total, batch_size and world must be positive, phase 0 or 1");
  if (!perm || !advantages || !slot || (phase == 1 && !slots)) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  const unsigned blocks = (unsigned)((total + (int64_t)batch_size - 1) / batch_size);
  hipLaunchKernelGGL(upkie::ppo_adv_partials_kernel, dim3(blocks), dim3(upkie::PPO_ADV_THREADS), 0, (hipStream_t)stream, total, batch_size, perm,
                     advantages, phase, slots, world, slot);
  return launch_status();
}

extern "C" int upkie_ppo_advantage_finish(int32_t total, int32_t batch_size, int32_t normalize, const double* slots, int32_t world,
                                          double* adv_stats, void* stream) {
  if (total < 1 || batch_size < 1 || world < 1) return fail(UPKIE_ERR_INVALID_ARGUMENT, "total, batch_size and world must be positive");
  if (!slots || !adv_stats) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  const int M = (int)((total + (int64_t)batch_size - 1) / batch_size);
  hipLaunchKernelGGL(upkie::ppo_adv_finish_kernel, dim3((unsigned)((M + upkie::PPO_THREADS - 1) / upkie::PPO_THREADS)), dim3(upkie::PPO_THREADS), 0,
                     (hipStream_t)stream, total, batch_size, M, normalize ? 1 : 0, slots, world, adv_stats);
  return launch_status();
}

// ---- the distillation update (include/upkie_hip.h; distill.hpp)
static int check_distill_shape(const UpkieMlpShape* shape, upkie::PpoPlan* plan) {
  if (!shape) return fail(UPKIE_ERR_INVALID_ARGUMENT, "null shape");
  if (upkie::mlp_layout(*shape, nullptr) < 0) return (int)upkie_mlp_packed_words(shape);  // (sets the message)
  if (!upkie::distill_plan(*shape, plan))
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "distillation needs a student with a critic (critic_layers > 0), as PPO does");
  return UPKIE_OK;
}

extern "C" int64_t upkie_distill_workspace_bytes(const UpkieMlpShape* shape, int32_t max_minibatch) {
  upkie::PpoPlan plan;
  if (check_distill_shape(shape, &plan)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (max_minibatch < 1) return fail(UPKIE_ERR_INVALID_ARGUMENT, "max_minibatch must be positive");
  return upkie::ppo_workspace_bytes(plan, upkie::ppo_grid(plan, max_minibatch));
}

extern "C" int upkie_distill_minibatch_update(const UpkieMlpShape* shape, int32_t total, int32_t minibatch_start, int32_t minibatch_size,
                                              int32_t max_minibatch, const int32_t* perm, const float* obs, const float* labels, float* packed,
                                              float* adam_m, float* adam_v, double* adam_scalars, double max_grad_norm, double adam_beta1,
                                              double adam_beta2, double adam_eps, int32_t obs_normalized, void* workspace, float* stats,
                                              void* stream) {
  upkie::PpoPlan plan;
  if (check_distill_shape(shape, &plan)) return UPKIE_ERR_INVALID_ARGUMENT;
  if (!(max_grad_norm > 0.0) || !(adam_eps > 0.0) || !(adam_beta1 >= 0.0 && adam_beta1 < 1.0) || !(adam_beta2 >= 0.0 && adam_beta2 < 1.0))
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "max_grad_norm and adam_eps must be positive, adam betas in [0, 1)");
  if (total < 1 || minibatch_size < 1 || max_minibatch < 1 || minibatch_start < 0 || minibatch_size > max_minibatch ||
      (int64_t)minibatch_start + minibatch_size > total)
    return fail(UPKIE_ERR_INVALID_ARGUMENT,
                "minibatch out of range: 0 <= minibatch_start, 1 <= minibatch_size <= max_minibatch, start + size <= total");
  if ((int64_t)total * (shape->obs_dim > shape->act_dim ? shape->obs_dim : shape->act_dim) > INT_MAX)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "total * obs_dim (or act_dim) must stay below 2^31");
  if (!perm || !obs || !labels || !packed || !adam_m || !adam_v || !adam_scalars || !workspace || !stats)
    return fail(UPKIE_ERR_INVALID_ARGUMENT, "null argument");
  if ((uintptr_t)adam_scalars % 8 != 0) return fail(UPKIE_ERR_INVALID_ARGUMENT, "adam_scalars must be 8-byte aligned");
  if (no_device()) return UPKIE_ERR_NO_DEVICE;
  upkie::PpoDev P{};
  upkie::mlp_layout(*shape, &P.net);
  P.stage[0] = plan.stage[0], P.stage[1] = plan.stage[1];
  P.train_off = plan.train_off, P.train_words = plan.train_words;  // (the actor's span: distill.hpp)
  P.nw = plan.nw, P.tile_floats = plan.tile_floats, P.fold_blocks = plan.fold_blocks;
  P.part_stride = plan.train_words, P.stat_stride = upkie::PPO_STATS;
  P.mb_start = minibatch_start, P.mb_size = minibatch_size, P.count = minibatch_size;
  P.grid = upkie::ppo_grid(plan, minibatch_size);
  P.obs_normalized = obs_normalized ? 1 : 0;
  P.max_grad_norm = (float)max_grad_norm, P.beta1 = (float)adam_beta1, P.beta2 = (float)adam_beta2, P.adam_eps = (float)adam_eps;
  P.perm = perm, P.obs = obs, P.actions = labels;  // (the behaviour-cloning head reads the labels where PPO's reads the actions)
  P.packed = packed, P.m = adam_m, P.v = adam_v, P.scalars = adam_scalars, P.ctrl = nullptr, P.stats = stats;
  const int ws_grid = upkie::ppo_grid(plan, max_minibatch);  // (the workspace's layout)
  char* ws = (char*)workspace;
  P.ticket = (unsigned*)ws;
  P.header = (float*)ws;
  P.partials = (float*)(ws + upkie::PPO_HEADER_BYTES);
  P.stat_partials = (double*)(ws + upkie::ppo_stat_partials_at(plan, ws_grid));
  P.grad = (float*)(ws + upkie::ppo_grad_at(plan, ws_grid));
  P.sq_partials = (double*)(ws + upkie::ppo_sq_at(plan, ws_grid));
  const hipStream_t s = (hipStream_t)stream;
  const int status = for_mlp_instance(*shape, [&](auto w, auto act) {
    auto kernel = upkie::ppo_grad_kernel<w(), act(), true>;
    if (plan.lds_bytes > upkie::PPO_LDS_BUDGET) {  // (as ppo_abi.hip raises it: once per instantiation, to what any valid shape can need)
      static const hipError_t raised = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, upkie::PPO_LDS_MAX);
      if (raised != hipSuccess) return launch_status(raised);
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)P.grid), dim3(64 * P.nw), (size_t)plan.lds_bytes, s, P);
    return launch_status();
  });
  if (status != UPKIE_OK) return status;
  hipLaunchKernelGGL(upkie::distill_fold_kernel, dim3((unsigned)P.fold_blocks), dim3(upkie::PPO_THREADS), 0, s, P);
  hipLaunchKernelGGL(upkie::ppo_adam_kernel, dim3((unsigned)P.fold_blocks), dim3(upkie::PPO_THREADS), 0, s, P);
  return launch_status();
}
