// distill_mix.hpp -- the DAgger mix of a distillation rollout step (include/upkie_hip.h, "Policy distillation"): per env
// one Philox block decides whether the teacher's label or the student's action drives the env this step, and the chosen
// row is clamped to the action bounds. One launch per step, one env per lane. The kernel only selects and clamps, so it
// is exact; the draw is keyed by the GLOBAL env id under the handle's seed, like the episode events' and the task
// targets', so 64 envs are two shards of 32 bit for bit. Included by upkie_hip.hip only (the handle's DevConfig).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "random.hpp"
#include "step_kernels.hpp"

namespace upkie {

// threshold: ONE device word, llround(beta 2^24): the teacher drives iff (word 0 >> 8) < threshold (0: never, 2^24:
// always). In device memory so that a beta schedule moves under a captured rollout.
__global__ __launch_bounds__(64) void distill_mix_kernel(DevConfig C, int act_dim, const unsigned* __restrict__ threshold,
                                                         const float* __restrict__ label, const float* __restrict__ student,
                                                         const float* __restrict__ low, const float* __restrict__ high,
                                                         unsigned* __restrict__ calls, float* __restrict__ applied, uint8_t* __restrict__ drove) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= C.num_envs) return;
  const unsigned call = calls[e];
  const unsigned lo = C.env_lo + (unsigned)e;
  const unsigned hi = C.env_hi + (lo < C.env_lo ? 1u : 0u);
  unsigned r[4];
  philox4x32_10(lo, hi, call, (unsigned)STREAM_DISTILL << 24, C.seed_lo, C.seed_hi, r);
  calls[e] = call + 1u;
  const bool teacher = (r[0] >> 8) < threshold[0];
  const float* __restrict__ src = (teacher ? label : student) + (size_t)e * act_dim;
  float* __restrict__ dst = applied + (size_t)e * act_dim;
  for (int a = 0; a < act_dim; ++a) dst[a] = fminf(fmaxf(src[a], low[a]), high[a]);
  drove[e] = teacher ? 1 : 0;
}

}  // namespace upkie
