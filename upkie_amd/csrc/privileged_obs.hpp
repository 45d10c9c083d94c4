// privileged_obs.hpp -- the row the critic of an asymmetric actor-critic reads ("privileged observations"), assembled in
// ONE launch per env step from what the device already holds: the raw next observation, the command the env received,
// the force the next step will apply and the link scales this episode drew (include/upkie_hip.h states the row and its
// terminal form; Python: upkie_amd/privileged.py). Data movement only: every output word is a copy of one input word.
//
// Work split: a block takes PRIVILEGED_ENVS = 64 envs. The row-major sources (next_obs, final_obs, command: [N][*]) are
// read and the [N][row_dim] outputs written element-wise, thread i of a pass = word i of the tile's rows, so loads and
// stores are coalesced. The column-major sources (force, link_scale: [*][N]) would be strided that way; they are first
// staged into LDS with adjacent lanes on adjacent envs (one wave per column: 64 consecutive words), then read from LDS
// in the element-wise pass. The terminal row keeps the OLD observation word for everything but the observation segment:
// the thread that writes observation[n][k] reads it first, so no other thread's write can come between.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/upkie_hip.h"

namespace upkie {

enum {
  PRIVILEGED_THREADS = 256,
  PRIVILEGED_ENVS = 64,          // envs of a block: one wave per staged column
  PRIVILEGED_MAX_COLUMNS = 32,   // staged ([*][N]) words of a row: 3 force words + UPKIE_MAX_LINKS scales fit
};

struct PrivilegedDev {
  int num_envs, obs_dim, act_dim, row_dim, num_segments, reset, columns;
  int kind[UPKIE_PRIVILEGED_MAX_SEGMENTS], start[UPKIE_PRIVILEGED_MAX_SEGMENTS], count[UPKIE_PRIVILEGED_MAX_SEGMENTS];
  int column[UPKIE_PRIVILEGED_MAX_SEGMENTS];  // first staged column of a force / link_scale segment
  const float* next_obs;
  const float* final_obs;
  const float* command;
  const float* force;
  const float* link_scale;
  const int32_t* links;
  const uint8_t* terminated;  // (reset: the mask)
  const uint8_t* truncated;
  float* observation;
  float* final_observation;
};

// Fills start / column / row_dim / columns from kind / count; false when a segment is out of range.
inline bool privileged_layout(PrivilegedDev& P) {
  if (P.num_segments < 1 || P.num_segments > UPKIE_PRIVILEGED_MAX_SEGMENTS) return false;
  int row = 0, cols = 0;
  for (int k = 0; k < P.num_segments; ++k) {
    const int n = P.count[k];
    int limit = 0;
    switch (P.kind[k]) {
      case UPKIE_PRIVILEGED_OBSERVATION: limit = P.obs_dim; break;
      case UPKIE_PRIVILEGED_COMMAND: limit = P.act_dim; break;
      case UPKIE_PRIVILEGED_PUSH_FORCE: limit = 3; break;
      case UPKIE_PRIVILEGED_LINK_SCALE: limit = UPKIE_MAX_LINKS; break;
      default: return false;
    }
    if (n < 1 || n > limit) return false;
    P.start[k] = row, row += n;
    P.column[k] = cols;
    if (P.kind[k] == UPKIE_PRIVILEGED_PUSH_FORCE || P.kind[k] == UPKIE_PRIVILEGED_LINK_SCALE) cols += n;
  }
  if (row > 256 || cols > PRIVILEGED_MAX_COLUMNS) return false;
  P.row_dim = row, P.columns = cols;
  return true;
}

#if defined(__HIPCC__)

__global__ __launch_bounds__(PRIVILEGED_THREADS) void privileged_observation_kernel(const PrivilegedDev P) {
  __shared__ float tile[PRIVILEGED_MAX_COLUMNS][PRIVILEGED_ENVS + 1];
  const int env0 = blockIdx.x * PRIVILEGED_ENVS;
  const int envs = P.num_envs - env0 < PRIVILEGED_ENVS ? P.num_envs - env0 : PRIVILEGED_ENVS;
  const size_t N = (size_t)P.num_envs;
  // the [*][N] sources: column c of the stage by one wave at a time, lane = env
  for (int i = threadIdx.x; i < P.columns * PRIVILEGED_ENVS; i += PRIVILEGED_THREADS) {
    const int c = i / PRIVILEGED_ENVS, e = i % PRIVILEGED_ENVS;
    if (e < envs) {
      float v = 0.f;
      for (int s = 0; s < P.num_segments; ++s) {
        const int j = c - P.column[s];
        if (j < 0 || j >= P.count[s]) continue;
        if (P.kind[s] == UPKIE_PRIVILEGED_PUSH_FORCE) v = P.force[(size_t)j * N + env0 + e];
        else if (P.kind[s] == UPKIE_PRIVILEGED_LINK_SCALE) v = P.link_scale[(size_t)P.links[j] * N + env0 + e];
      }
      tile[c][e] = v;
    }
  }
  __syncthreads();
  // the rows, element-wise
  for (int i = threadIdx.x; i < envs * P.row_dim; i += PRIVILEGED_THREADS) {
    const int e = i / P.row_dim, k = i - e * P.row_dim;
    const int n = env0 + e;
    const size_t at = (size_t)n * P.row_dim + k;
    int s = 0;
    while (s + 1 < P.num_segments && k >= P.start[s + 1]) ++s;
    const int j = k - P.start[s];
    const uint8_t flag = (P.terminated && P.terminated[n] != 0) || (P.truncated && P.truncated[n] != 0) ? 1 : 0;
    float v, fin;
    if (P.kind[s] == UPKIE_PRIVILEGED_OBSERVATION) {
      v = P.next_obs[(size_t)n * P.obs_dim + j];
      fin = !P.reset && flag && P.final_obs ? P.final_obs[(size_t)n * P.obs_dim + j] : v;
    } else {
      v = P.kind[s] == UPKIE_PRIVILEGED_COMMAND ? P.command[(size_t)n * P.act_dim + j] : tile[P.column[s] + j][e];
      fin = !P.reset && flag ? P.observation[at] : v;  // (the old word, read before this thread overwrites it)
    }
    if (P.reset) {
      if (!P.terminated || flag) P.observation[at] = v;
    } else {
      P.final_observation[at] = fin;
      P.observation[at] = v;
    }
  }
}

#endif  // __HIPCC__

}  // namespace upkie
