// distill.hpp -- policy distillation on the device: one minibatch of a behaviour-cloning update of an MlpActorCritic's
// ACTOR tower (L = 1/(B A) sum_j sum_a (mean_a(obs_j) - label_ja)^2, torch's mse_loss of the Gaussian's unclamped mean
// against the label; its gradient, clip_grad_norm_, Adam) in three launches. include/upkie_hip.h states the arithmetic;
// Python: upkie_amd/distill.py. The DAgger mix of a rollout step is distill_mix.hpp.
//
// Launch A is ppo.hpp's gradient kernel with BC = true: the same gather through the permutation, ppo_stage_x, forward
// (mlp_dense / mlp_dot), ppo_dx, ppo_dw_mfma / ppo_dw_dot, per-block partials and fp64 loss sum; only the head differs
// (dZ = 2 (mean - label) / (B A)), the critic tower does not run and log_std gets nothing.
//
// What gets no gradient, and how: the plan's trainable range is the ACTOR's words alone -- train_off is the actor's first
// weight word (right after log_std), train_words ends where the critic begins. The partials, the fold and Adam range over
// exactly that span, every word of which the first chunk of every block writes (as in PPO: each fragment, bias and head
// word has one owning thread; the padding words are inside a written fragment or bias row -- ppo_dw_mfma covers all
// out_tiles * in_tiles * 256 weight and 16 * out_tiles bias words, ppo_dw_dot the 3 spare words of a dot head's bias, as
// zeros -- so the span needs no zeroed workspace: tests/test_distill_gpu.py runs the update on partials filled with NaN
// bits). So no partial word is left uninitialised and none outside the span exists: log_std, every
// critic word and the fixed words before log_std are never read-modified or written, and their m and v stay as they
// were (0 under a fresh optimiser state).
//
// Launch B (distill_fold_kernel) has ppo_fold_kernel's structure -- word i summed over the partials in block order, a
// fixed LDS tree per block, the ticket, the last block's thread 0 alone in a fixed order -- without the entropy term and
// with the statistics row (loss, ||g|| before the clip, the clip coefficient). Launch C is ppo_adam_kernel unchanged.
// lr and t are the two fp64 words of `scalars` in device memory (the control block's first two): a captured update
// follows a learning-rate schedule with no re-capture.
#pragma once

#include "ppo.hpp"

namespace upkie {

enum { DISTILL_STATS = 3 };  // the statistics row: loss, ||g|| before the clip, the clip coefficient

// ppo_plan's stage layout and waves per block (the shapes it accepts, and no others) with the actor's span as the
// trainable range; the workspace layout functions of ppo.hpp then apply as they are.
inline bool distill_plan(const UpkieMlpShape& s, PpoPlan* plan) {
  PpoPlan p{};
  if (!ppo_plan(s, &p)) return false;
  MlpDev d;
  mlp_layout(s, &d);
  p.train_off = d.actor.hidden[0].w_off;
  p.train_words = d.critic.hidden[0].w_off - p.train_off;
  const int64_t cap = PPO_PARTIAL_CAP_BYTES / (4 * (int64_t)p.train_words);
  p.grid_cap = cap < 1 ? 1 : cap > PPO_MAX_GRID ? PPO_MAX_GRID : (int)cap;
  p.fold_blocks = (p.train_words + PPO_THREADS - 1) / PPO_THREADS;
  if (plan) *plan = p;
  return true;
}

#if defined(__HIPCC__)

// Launch B: fold the partials over the actor's words, ||g||^2 per block, and the last block's scalars.
__global__ __launch_bounds__(PPO_THREADS) void distill_fold_kernel(const PpoDev P) {
  __shared__ double lds[PPO_THREADS + 1];
  const int tid = threadIdx.x, i = blockIdx.x * PPO_THREADS + tid;
  double sq = 0.0;
  if (i < P.train_words) {
    const float s = fold_in_block_order(P.partials + i, P.grid, P.part_stride);
    P.grad[i] = s;
    sq = (double)s * (double)s;
  }
  lds[tid] = sq;
  lds_tree_sum<PPO_THREADS>(tid, lds);
  if (tid == 0) P.sq_partials[blockIdx.x] = lds[0];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid != 0 || !ticket_draw(P.ticket, P.fold_blocks)) return;  // (thread 0 of the last block goes on alone)
  __hip_atomic_store(P.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  double total = 0.0;
  for (int b = 0; b < P.fold_blocks; ++b) total += P.sq_partials[b];
  const double norm = sqrt(total);
  const double coef = fmin(1.0, (double)P.max_grad_norm / (norm + 1e-6));
  double sum = 0.0;
  for (int b = 0; b < P.grid; ++b) sum += P.stat_partials[(size_t)b * P.stat_stride];
  P.stats[0] = (float)(sum / ((double)P.count * (double)P.net.act_dim));
  P.stats[1] = (float)norm;
  P.stats[2] = (float)coef;
  const double t = P.scalars[1] + 1.0;
  P.scalars[1] = t;
  P.header[4] = (float)coef;
  P.header[5] = (float)(P.scalars[0] / (1.0 - pow((double)P.beta1, t)));
  P.header[6] = (float)sqrt(1.0 - pow((double)P.beta2, t));
}

#endif  // __HIPCC__

}  // namespace upkie
