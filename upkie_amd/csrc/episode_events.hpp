// episode_events.hpp -- what happens to an env BETWEEN two steps of a rollout, decided on the device: random pushes with
// a per-env schedule and a fresh draw of the link inertias when an episode ends (include/upkie_hip.h, "Episode events",
// states the arithmetic). One launch per env step, one env per lane on the [word][N] layout: every load and store of a
// wavefront is contiguous. Included by upkie_hip.hip only: it needs the handle's DevConfig (seed, global env ids) and
// DevLinks, and fuse_links of host_setup.hpp. The step kernels are not touched: they read the force buffer and the
// inertial records this kernel writes, as they read any the caller installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "host_setup.hpp"

namespace upkie {

// UpkieEpisodeEvents as the kernels read it (events_params, upkie_hip.hip, checks and converts)
struct EventsParams {
  unsigned threshold;   // a push starts iff (word 0 >> 8) < threshold: llround(push_prob * 2^24)
  int steps_min;        // steps a push is held: steps_min + (word 3 >> 8) % steps_span
  unsigned steps_span;  // steps_max - steps_min + 1
  float norm_min, norm_max;
  float variation;  // of the link factors
};

// The link factors of (env e, episode) and the records they fuse into: body_inertials_kernel's draw, with the episode
// as counter word 2 (0 there).
__device__ __forceinline__ void events_redraw_inertials(const DevConfig& C, const DevLinks& L, int e, unsigned episode, float variation,
                                                        float* __restrict__ records, float* __restrict__ link_scale) {
  const int B = C.num_envs;
  float f[UPKIE_MAX_LINKS];
#pragma unroll
  for (int blk = 0; blk < UPKIE_MAX_LINKS / 4; ++blk) {
    float u[4];
    philox_uniform4(C, (unsigned)e, episode, STREAM_INERTIA, blk, u);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int l = 4 * blk + i;
      f[l] = (l < L.count && L.randomized[l]) ? 1.f + uniform(-variation, variation, u[i]) : 1.f;
      link_scale[(size_t)l * B + e] = f[l];
    }
  }
  fuse_links(L, f, records + e, (size_t)B);
}

// records / link_scale null: no inertia randomisation. terminated / truncated: either may be null (0).
__global__ __launch_bounds__(64) void episode_events_kernel(DevConfig C, DevLinks L, EventsParams P, const uint8_t* __restrict__ terminated,
                                                            const uint8_t* __restrict__ truncated, unsigned* __restrict__ calls,
                                                            int* __restrict__ remaining, unsigned* __restrict__ pushes,
                                                            unsigned* __restrict__ episodes, float* __restrict__ force,
                                                            float* __restrict__ records, float* __restrict__ link_scale) {
  const int B = C.num_envs;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B) return;
  // 1. the call's own block: every env, every call, whatever the others do
  const unsigned call = calls[e];
  const unsigned lo = C.env_lo + (unsigned)e;
  const unsigned hi = C.env_hi + (lo < C.env_lo ? 1u : 0u);
  unsigned r[4];
  philox4x32_10(lo, hi, call, (unsigned)STREAM_EVENTS << 24, C.seed_lo, C.seed_hi, r);
  calls[e] = call + 1u;
  int left = remaining[e];
  // 2. the episode ended: its push ends with it, the next one gets links of its own (rare and heavy: a wavefront without
  // a finisher skips it as a whole)
  const bool done = ((terminated ? terminated[e] : 0) | (truncated ? truncated[e] : 0)) != 0;
  if (done) {
    const unsigned episode = episodes[e] + 1u;
    episodes[e] = episode;
    left = 0;
    if (records) events_redraw_inertials(C, L, e, episode, P.variation, records, link_scale);
  }
  // 3. one step of a held force is over
  if (left > 0) left -= 1;
  // 4. a free step: a push starts or the force is zero; 5. otherwise the force stays as it is
  if (left == 0) {
    float fx = 0.f, fy = 0.f;
    if ((r[0] >> 8) < P.threshold) {
      const unsigned k = pushes[e];
      float u[4];
      philox_uniform4(C, (unsigned)e, k, STREAM_PUSH, 0u, u);  // push number k of this env, as push_kernel draws it
      const float norm = uniform(P.norm_min, P.norm_max, u[0]);
      float sn, cs;
      sincosf(6.283185307179586f * u[1], &sn, &cs);
      fx = norm * cs;
      fy = norm * sn;
      pushes[e] = k + 1u;
      left = P.steps_min + (int)((r[3] >> 8) % P.steps_span);
    }
    force[e] = fx;
    force[(size_t)B + e] = fy;
    force[(size_t)2 * B + e] = 0.f;
  }
  remaining[e] = left;
}

// mask null: every env
__global__ __launch_bounds__(64) void episode_events_reset_kernel(DevConfig C, DevLinks L, EventsParams P, const uint8_t* __restrict__ mask,
                                                                  unsigned* __restrict__ calls, int* __restrict__ remaining,
                                                                  unsigned* __restrict__ pushes, unsigned* __restrict__ episodes,
                                                                  float* __restrict__ force, float* __restrict__ records,
                                                                  float* __restrict__ link_scale) {
  const int B = C.num_envs;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B) return;
  if (mask && !mask[e]) return;
  calls[e] = 0u;
  remaining[e] = 0;
  pushes[e] = 0u;
  episodes[e] = 0u;
  force[e] = 0.f;
  force[(size_t)B + e] = 0.f;
  force[(size_t)2 * B + e] = 0.f;
  if (records) events_redraw_inertials(C, L, e, 0u, P.variation, records, link_scale);
}

}  // namespace upkie
