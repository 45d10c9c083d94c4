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

// The push curriculum (include/upkie_hip.h, "Push curriculum"): the words of the device block `settings`, read at every
// call, and the per-env state the levelled instantiation carries. Without levels the state is empty and P is the launch's.
enum {
  EVENTS_THRESHOLD = 0, EVENTS_NORM_MIN = 1, EVENTS_NORM_MAX = 2, EVENTS_STEPS_MIN = 3, EVENTS_STEPS_SPAN = 4, EVENTS_LEVELS = 5,
  EVENTS_UP = 6, EVENTS_DOWN = 7, EVENTS_MIN_PUSHES = 8
};
static_assert(EVENTS_MIN_PUSHES + 1 == UPKIE_EVENTS_SETTINGS_WORDS, "the block's words");

template <bool LEVELS>
struct EventsLevels {};
template <>
struct EventsLevels<true> {
  const unsigned* __restrict__ settings;  // [UPKIE_EVENTS_SETTINGS_WORDS]
  unsigned* __restrict__ level;
  unsigned* __restrict__ episode_pushes;
  float* __restrict__ difficulty;
};

// the fraction level l of L scales the norm range by: 1 at the top, which includes L = 0 (no division then)
__device__ __forceinline__ float events_difficulty(unsigned l, unsigned L) { return l >= L ? 1.f : (float)l / (float)L; }

// (every word of the block is the same for all lanes: scalar loads)
__device__ __forceinline__ void events_read_settings(const unsigned* __restrict__ w, EventsParams& P) {
  P.threshold = w[EVENTS_THRESHOLD];
  P.norm_min = __uint_as_float(w[EVENTS_NORM_MIN]);
  P.norm_max = __uint_as_float(w[EVENTS_NORM_MAX]);
  P.steps_min = (int)w[EVENTS_STEPS_MIN];
  P.steps_span = w[EVENTS_STEPS_SPAN] ? w[EVENTS_STEPS_SPAN] : 1u;  // (a damaged block does not divide by zero)
}

// records / link_scale null: no inertia randomisation. terminated / truncated: either may be null (0). LEVELS: the push
// settings come from the device block (P carries the variation alone) and every env has a difficulty level.
template <bool LEVELS>
__global__ __launch_bounds__(64) void episode_events_kernel(DevConfig C, DevLinks L, EventsParams P, EventsLevels<LEVELS> S,
                                                            const uint8_t* __restrict__ terminated, const uint8_t* __restrict__ truncated,
                                                            unsigned* __restrict__ calls, int* __restrict__ remaining,
                                                            unsigned* __restrict__ pushes, unsigned* __restrict__ episodes,
                                                            float* __restrict__ force, float* __restrict__ records,
                                                            float* __restrict__ link_scale) {
  const int B = C.num_envs;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B) return;
  unsigned top = 0u, level = 0u, in_episode = 0u;  // (top: L, the highest level)
  if constexpr (LEVELS) {
    events_read_settings(S.settings, P);
    top = S.settings[EVENTS_LEVELS];
    level = min(S.level[e], top);
    in_episode = S.episode_pushes[e];
  }
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
  const bool fell = LEVELS && terminated && terminated[e] != 0;
  const bool done = ((terminated ? terminated[e] : 0) | (truncated ? truncated[e] : 0)) != 0;
  if (done) {
    if constexpr (LEVELS) {  // a fall demotes (and wins over the time limit), a survived episode that was pushed promotes
      if (fell)
        level -= min(level, S.settings[EVENTS_DOWN]);
      else if (in_episode >= S.settings[EVENTS_MIN_PUSHES])
        level = min(level + S.settings[EVENTS_UP], top);
      in_episode = 0u;
    }
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
      float norm_high = P.norm_max;
      if constexpr (LEVELS) {  // (the level this call left: a start on the call that ended an episode uses the new one)
        if (level < top) norm_high = fmaf(P.norm_max - P.norm_min, (float)level / (float)top, P.norm_min);
        in_episode += 1u;
      }
      const float norm = uniform(P.norm_min, norm_high, u[0]);
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
  if constexpr (LEVELS) {
    S.level[e] = level;
    S.episode_pushes[e] = in_episode;
    S.difficulty[e] = events_difficulty(level, top);
  }
}

// mask null: every env. LEVELS: the masked envs start at start_level.
template <bool LEVELS>
__global__ __launch_bounds__(64) void episode_events_reset_kernel(DevConfig C, DevLinks L, EventsParams P, EventsLevels<LEVELS> S,
                                                                  unsigned start_level, const uint8_t* __restrict__ mask,
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
  if constexpr (LEVELS) {
    S.level[e] = start_level;
    S.episode_pushes[e] = 0u;
    S.difficulty[e] = events_difficulty(start_level, S.settings[EVENTS_LEVELS]);
  }
}

// counts[l] += the envs at level l (a level above 255 counts at 255); counts is UPKIE_EVENTS_LEVELS_MAX + 1 words, zeroed
// by the entry point in front of the launch. Integer sums only: LDS bins per block, then one atomic per bin in use.
constexpr int EVENTS_COUNT_LANES = 256;
constexpr int EVENTS_COUNT_BLOCKS = 64;  // (at most: the envs beyond are taken by a grid stride)
__global__ __launch_bounds__(EVENTS_COUNT_LANES) void episode_events_level_counts_kernel(int B, const unsigned* __restrict__ level,
                                                                                         unsigned* __restrict__ counts) {
  __shared__ unsigned bins[UPKIE_EVENTS_LEVELS_MAX + 1];
  for (int l = threadIdx.x; l <= UPKIE_EVENTS_LEVELS_MAX; l += EVENTS_COUNT_LANES) bins[l] = 0u;
  __syncthreads();
  for (long long e = (long long)blockIdx.x * EVENTS_COUNT_LANES + threadIdx.x; e < B; e += (long long)gridDim.x * EVENTS_COUNT_LANES)
    atomicAdd(&bins[min(level[e], (unsigned)UPKIE_EVENTS_LEVELS_MAX)], 1u);
  __syncthreads();
  for (int l = threadIdx.x; l <= UPKIE_EVENTS_LEVELS_MAX; l += EVENTS_COUNT_LANES)
    if (bins[l]) atomicAdd(&counts[l], bins[l]);
}

}  // namespace upkie
