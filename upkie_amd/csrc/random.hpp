// random.hpp -- every random draw of the device code: the Philox4x32-10 rounds, the one list of stream tags, uniforms and
// normals from a block's words. Included by step_kernels.hpp, policy_mlp.hpp and agent_pipeline.hpp; includes none of them.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace upkie {

// Philox4x32-10 (Salmon et al., SC'11): counter = (env id lo/hi, episode, stream<<24 | block), key = seed: results do not
// depend on how envs are sharded. Host + device, and the high word of a product through 64 bits (what __umulhi compiles
// to), so that tests/host_harness.hip holds the rounds to the Random123 known answers on a CPU.
__host__ __device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                                       unsigned (&out)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    unsigned hi0 = (unsigned)((0xD2511F53ull * c0) >> 32), lo0 = 0xD2511F53u * c0;
    unsigned hi1 = (unsigned)((0xCD9E8D57ull * c2) >> 32), lo1 = 0xCD9E8D57u * c2;
    unsigned n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Stream tags, the top byte of counter word 3: two draws can share a Philox block only under one tag, so every user of the
// rounds takes its tag from this one list. 0-3 are the simulator's (reset states, torque noise, per-episode inertias,
// pushes), under the sim's seed; the MLP policy's samples and the agent pipeline's noise count (env, call, 0) under their own;
// 6 is the episode events' schedule (env, call), under the sim's seed too (episode_events.hpp, which also redraws 2 per episode);
// 7 the task targets' (env, call), under the sim's seed: block 0 the schedule, blocks 1 and 2 the values (task_targets.hpp);
// 8 the distillation mix's (env, call), under the sim's seed: who drives the env this step (distill_mix.hpp).
enum {
  STREAM_RESET = 0, STREAM_NOISE = 1, STREAM_INERTIA = 2, STREAM_PUSH = 3, STREAM_POLICY = 4, STREAM_PIPELINE = 5, STREAM_EVENTS = 6,
  STREAM_TARGETS = 7, STREAM_DISTILL = 8
};

template <class ConfigT>
__device__ __forceinline__ void philox_uniform4(const ConfigT& C, unsigned env_local, unsigned episode, unsigned stream,
                                                unsigned block, float (&u)[4]) {
  unsigned lo = C.env_lo + env_local;
  unsigned hi = C.env_hi + (lo < C.env_lo ? 1u : 0u);
  unsigned r[4];
  philox4x32_10(lo, hi, episode, (stream << 24) | block, C.seed_lo, C.seed_hi, r);
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = (float)(r[i] >> 8) * (1.0f / 16777216.0f);
}

// Box-Muller on two Philox words: two standard normals, the cosine one first. u1 = ((ra >> 8) + 1) / 2^24 lies in
// (0, 1] (never 0: the logarithm is finite), u2 = (rb >> 8) / 2^24 in [0, 1).
__device__ __forceinline__ void box_muller(unsigned ra, unsigned rb, float& z_cos, float& z_sin) {
  const float u1 = ((float)(ra >> 8) + 1.0f) * (1.0f / 16777216.0f);
  const float u2 = (float)(rb >> 8) * (1.0f / 16777216.0f);
  const float radius = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  z_cos = radius * cs;
  z_sin = radius * sn;
}

// Six standard normals for (env, step, slot): Box-Muller on two Philox blocks. slot = substep index (control noise) or
// NOISE_SLOT_MEASUREMENT. (box_muller's arithmetic, written out: through the helper the compiler schedules the Philox
// rounds of the step kernels differently, and their instruction streams are held fixed.)
#define NOISE_SLOT_MEASUREMENT 0x7fffu
template <class ConfigT>
__device__ __forceinline__ void philox_normal6(const ConfigT& C, unsigned env_local, unsigned step, unsigned slot, float (&z)[6]) {
  unsigned lo = C.env_lo + env_local;
  unsigned hi = C.env_hi + (lo < C.env_lo ? 1u : 0u);
  unsigned r[8];
#pragma unroll
  for (unsigned k = 0; k < 2; ++k) {
    unsigned q[4];
    philox4x32_10(lo, hi, step, ((unsigned)STREAM_NOISE << 24) | (slot * 2u + k), C.seed_lo, C.seed_hi, q);
    r[4 * k] = q[0]; r[4 * k + 1] = q[1]; r[4 * k + 2] = q[2]; r[4 * k + 3] = q[3];
  }
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    float u1 = ((float)(r[2 * p] >> 8) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
    float u2 = (float)(r[2 * p + 1] >> 8) * (1.0f / 16777216.0f);
    float radius = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    z[2 * p] = radius * cs;
    z[2 * p + 1] = radius * sn;
  }
}

}  // namespace upkie
