// policy_mlp.hpp -- the policy side of a rollout step in ONE launch: an SB3-style MLP actor-critic (separate actor and
// critic towers, tanh or ReLU, diagonal Gaussian with a learned log_std, optional frozen VecNormalize statistics) for a
// batch of envs, on fp32 MFMA (v_mfma_f32_16x16x4_f32: exact fp32, bit for bit a k-ordered fmaf chain).
//
// Mapping. Every layer is computed transposed, H^T = W . X^T: A = weights (16 output units x 4 k), B = activations
// (4 k x 16 envs). Lane l of a wave holds env l & 15; its accumulator i of output tile o is unit 16o + 4(l >> 4) + i.
// The k order of a sum is free, so k-step s of input tile t of a hidden layer takes units {16t + 4q + s : q = 0..3}:
// lane group q's B operand of that step is then exactly its own accumulator s of tile t, and the output of one layer
// feeds the next with no LDS round trip and no lane movement. Only the weight packing (layout below, Python:
// upkie_amd/policies.py) knows that order. The first layer reads the observation in natural order (k-step s of tile t:
// elements 16t + 4s + q), so that a 4-word observation costs one k-step per output tile, not four.
//
// Work split: one block of two waves per tile of 16 envs; wave 0 runs the actor (and writes the normalised
// observation), wave 1 the critic. Output tiles are processed in pairs (two independent accumulators in flight: the
// 16x16x4 MFMA issues every 32 cycles and has a 40-cycle dependent latency). One-row heads (the value, a one-dimensional
// action) are VALU dot products: 4 units per lane per tile, then two cross-lane sums (lanes l ^ 16, l ^ 32).
//
// Register arrays are indexed by compile-time constants only (full unrolls to the width class W with wave-uniform run
// time guards): the kernel is templated on W in {16, 32, 64, 128, 256} and on the activation, 10 instantiations.
//
// Packed weight buffer (fp32 words, every block a multiple of 4 words; Dp = obs_dim rounded up to 4, At = ceil(act_dim
// / 16), P = 2 when W >= 32 else 1, tiles(w) = ceil(w / 16), out tiles of an MFMA layer rounded up to a multiple of P):
//   obs_mean[Dp], obs_std[Dp]            (std = sqrt(var + eps); ignored unless shape->normalize)
//   action_low[16 At], action_high[16 At], log_std[16 At]
//   actor:  per hidden layer: weights[out_tiles][in_tiles][64 lanes][4 k-steps], bias[out_tiles][16]
//           head: act_dim == 1: weights[in_tiles][16], bias[4]; otherwise an MFMA layer of act_dim outputs
//   critic: per hidden layer as above; head: weights[in_tiles][16], bias[4]
// Weight word (o, t, lane l, step s) of a layer is W[16o + (l & 15)][k], k = 16t + 4s + (l >> 4) in the first layer,
// 16t + 4(l >> 4) + s after it; zero where the unit or k is past the layer's width.
//
// Asymmetric shape (shape.critic_obs_dim = Dc > 0, the critic reads a row of its own; include/upkie_hip.h): W also
// covers Dc, the critic's first layer has tiles(Dc) input tiles in the first-layer order of its own width, and one more
// fixed block, critic_obs_mean[Dcp], critic_obs_std[Dcp] (Dcp = Dc rounded up to 4), sits between action_high and
// log_std. Wave 1 then loads critic_obs with that width and those statistics; with Dc = 0 MlpDev's critic fields repeat
// the actor's and the kernel's arithmetic is word for word the symmetric one.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/upkie_hip.h"
#include "random.hpp"

namespace upkie {

struct MlpLayerDev {
  int w_off, b_off;  // words into the packed buffer
  int in_tiles, out_tiles;  // (out_tiles padded to the pair size; 0 and b_off = bias word for a dot head)
};

struct MlpTowerDev {
  int layers;
  MlpLayerDev hidden[UPKIE_MLP_MAX_LAYERS];
  MlpLayerDev head;
  int head_dot;  // one output row: VALU dot product
};

struct MlpDev {
  int num_envs, obs_dim, act_dim, act_tiles, normalize;
  float clip_obs;
  int mean_off, std_off, low_off, high_off, log_std_off;
  int critic_obs_dim, critic_mean_off, critic_std_off;  // the critic's input: the actor's (obs_dim, mean_off, std_off) for a symmetric shape
  MlpTowerDev actor, critic;
  int run_actor, run_critic, sample;
  unsigned seed_lo, seed_hi;
};

struct MlpOutputs {
  float* norm_obs;
  float* norm_critic_obs;  // asymmetric shapes: the critic's normalised row (written by wave 1)
  float* mean;
  float* action;
  float* env_action;
  float* value;
  float* log_prob;
};

// Width class of a shape (the template argument W), 0 when a dimension is out of range.
inline int mlp_width_class(const UpkieMlpShape& s) {
  int w = s.obs_dim > s.act_dim ? s.obs_dim : s.act_dim;
  w = s.critic_obs_dim > w ? s.critic_obs_dim : w;
  for (int i = 0; i < s.actor_layers && i < UPKIE_MLP_MAX_LAYERS; ++i) w = s.actor_widths[i] > w ? s.actor_widths[i] : w;
  for (int i = 0; i < s.critic_layers && i < UPKIE_MLP_MAX_LAYERS; ++i) w = s.critic_widths[i] > w ? s.critic_widths[i] : w;
  for (int c = 16; c <= 256; c *= 2)
    if (w <= c) return c;
  return 0;
}

// Offsets of the packed buffer (layout above) into `dev`; returns its length in words, or -1 for a shape out of range.
inline int64_t mlp_layout(const UpkieMlpShape& s, MlpDev* dev) {
  if (s.obs_dim < 1 || s.obs_dim > 256 || s.act_dim < 1 || s.act_dim > 64) return -1;
  if (s.activation != UPKIE_MLP_TANH && s.activation != UPKIE_MLP_RELU) return -1;
  if (s.actor_layers < 1 || s.actor_layers > UPKIE_MLP_MAX_LAYERS || s.critic_layers < 0 || s.critic_layers > UPKIE_MLP_MAX_LAYERS) return -1;
  for (int i = 0; i < s.actor_layers; ++i)
    if (s.actor_widths[i] < 1 || s.actor_widths[i] > 256) return -1;
  for (int i = 0; i < s.critic_layers; ++i)
    if (s.critic_widths[i] < 1 || s.critic_widths[i] > 256) return -1;
  if (s.normalize && !(s.clip_obs > 0.f)) return -1;
  if (s.critic_obs_dim < 0 || s.critic_obs_dim > 256 || (s.critic_obs_dim > 0 && s.critic_layers < 1)) return -1;
  const int W = mlp_width_class(s);
  if (W == 0) return -1;
  const int pair = W >= 32 ? 2 : 1;
  auto tiles = [](int w) { return (w + 15) / 16; };
  auto padded = [pair](int t) { return (t + pair - 1) / pair * pair; };
  MlpDev d{};
  int64_t off = 0;
  const int dp = (s.obs_dim + 3) / 4 * 4, at = tiles(s.act_dim);
  d.mean_off = (int)off, off += dp;
  d.std_off = (int)off, off += dp;
  d.low_off = (int)off, off += 16 * at;
  d.high_off = (int)off, off += 16 * at;
  const int dc = s.critic_obs_dim > 0 ? s.critic_obs_dim : s.obs_dim;
  d.critic_obs_dim = dc, d.critic_mean_off = d.mean_off, d.critic_std_off = d.std_off;
  if (s.critic_obs_dim > 0) {
    const int dcp = (dc + 3) / 4 * 4;
    d.critic_mean_off = (int)off, off += dcp;
    d.critic_std_off = (int)off, off += dcp;
  }
  d.log_std_off = (int)off, off += 16 * at;
  auto mfma_layer = [&](int in_tiles, int width) {
    MlpLayerDev L{};
    L.in_tiles = in_tiles;
    L.out_tiles = padded(tiles(width));
    L.w_off = (int)off, off += (int64_t)L.out_tiles * in_tiles * 256;
    L.b_off = (int)off, off += (int64_t)L.out_tiles * 16;
    return L;
  };
  auto dot_layer = [&](int in_tiles) {
    MlpLayerDev L{};
    L.in_tiles = in_tiles;
    L.w_off = (int)off, off += (int64_t)in_tiles * 16;
    L.b_off = (int)off, off += 4;
    return L;
  };
  auto tower = [&](MlpTowerDev& T, int inputs, int layers, const int32_t* widths, int outputs) {
    T.layers = layers;
    int in_tiles = tiles(inputs);
    for (int i = 0; i < layers; ++i) {
      T.hidden[i] = mfma_layer(in_tiles, widths[i]);
      in_tiles = tiles(widths[i]);
    }
    T.head_dot = outputs == 1;
    T.head = T.head_dot ? dot_layer(in_tiles) : mfma_layer(in_tiles, outputs);
  };
  tower(d.actor, s.obs_dim, s.actor_layers, s.actor_widths, s.act_dim);
  if (s.critic_layers > 0) tower(d.critic, dc, s.critic_layers, s.critic_widths, 1);
  d.obs_dim = s.obs_dim;
  d.act_dim = s.act_dim;
  d.act_tiles = at;
  d.normalize = s.normalize ? 1 : 0;
  d.clip_obs = s.clip_obs;
  if (dev) *dev = d;
  return off;
}

#if defined(__HIPCC__)

typedef float mlp_f4 __attribute__((ext_vector_type(4)));

template <int ACT>
__device__ __forceinline__ float mlp_activate(float x) {
  if constexpr (ACT == UPKIE_MLP_TANH) return tanhf(x);
  else return fmaxf(x, 0.f);
}

__device__ __forceinline__ mlp_f4 mlp_load4(const float* p) { return *reinterpret_cast<const mlp_f4*>(p); }

// One MFMA layer: out[o] = act(bias + W in) for the output tiles of L, two tiles per pass. FIRST: `in` is the
// observation (k-step s of tile t: elements 16t + 4s + q; steps past obs_dim are skipped), otherwise the previous
// layer's accumulators. ACTIVATE = false for the actor's mean head.
// The A fragments of up to CH input tiles are loaded back to back, unconditionally (tile index clamped to the layer's
// last tile: always inside the packing), before the MFMAs that use them: one L2 round trip per CH tiles instead of
// one per tile (behind the run-time tile guards the compiler cannot move a load ahead of the previous MFMAs).
template <int WT, int ACT, bool FIRST, bool ACTIVATE>
__device__ __forceinline__ void mlp_dense(const float* __restrict__ packed, const MlpLayerDev& L, int obs_dim, const float (&in)[WT][4],
                                          float (&out)[WT][4], int lane) {
  constexpr int PAIR = WT >= 2 ? 2 : 1;
  constexpr int CH = WT < 8 ? WT : 8;
  const int q = lane >> 4, last_t = L.in_tiles - 1;
  const float* __restrict__ wl = packed + L.w_off + lane * 4;
#pragma unroll
  for (int o = 0; o < WT; o += PAIR) {
    if (o < L.out_tiles) {
      mlp_f4 acc[PAIR];
#pragma unroll
      for (int p = 0; p < PAIR; ++p) acc[p] = mlp_load4(packed + L.b_off + 16 * (o + p) + 4 * q);
#pragma unroll
      for (int c = 0; c < WT; c += CH) {
        if (c < L.in_tiles) {
          mlp_f4 w[CH][PAIR];
#pragma unroll
          for (int j = 0; j < CH; ++j) {
            const int t = c + j < last_t ? c + j : last_t;
#pragma unroll
            for (int p = 0; p < PAIR; ++p) w[j][p] = mlp_load4(wl + ((o + p) * L.in_tiles + t) * 256);
          }
#pragma unroll
          for (int j = 0; j < CH; ++j) {
            const int t = c + j;
            if (t < L.in_tiles) {
#pragma unroll
              for (int s = 0; s < 4; ++s) {
                if (!FIRST || 16 * t + 4 * s < obs_dim) {
#pragma unroll
                  for (int p = 0; p < PAIR; ++p) acc[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][p][s], in[t][s], acc[p], 0, 0, 0);
                }
              }
            }
          }
        }
      }
#pragma unroll
      for (int p = 0; p < PAIR; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) out[o + p][i] = ACTIVATE ? mlp_activate<ACT>(acc[p][i]) : acc[p][i];
    }
  }
}

// One output row (value, or a one-dimensional action): every lane of an env column gets the full sum. (Loads
// unconditional and clamped to the last tile, as in mlp_dense.)
template <int WT>
__device__ __forceinline__ float mlp_dot(const float* __restrict__ packed, const MlpLayerDev& L, const float (&in)[WT][4], int lane) {
  const int q = lane >> 4, last_t = L.in_tiles - 1;
  mlp_f4 w[WT];
#pragma unroll
  for (int t = 0; t < WT; ++t) w[t] = mlp_load4(packed + L.w_off + 16 * (t < last_t ? t : last_t) + 4 * q);
  const float bias = packed[L.b_off];
  float part = 0.f;
#pragma unroll
  for (int t = 0; t < WT; ++t) {
    if (t < L.in_tiles) {
#pragma unroll
      for (int i = 0; i < 4; ++i) part = fmaf(w[t][i], in[t][i], part);
    }
  }
  part += __shfl_xor(part, 16);
  part += __shfl_xor(part, 32);
  return part + bias;
}

// Hidden layers of a tower, then its head into out (MFMA head) or *row (dot head).
template <int WT, int ACT>
__device__ __forceinline__ void mlp_tower(const float* __restrict__ packed, const MlpTowerDev& T, int obs_dim, const float (&x)[WT][4],
                                          float (&out)[WT][4], float* row, int lane) {
  float h[WT][4] = {}, g[WT][4] = {};
  mlp_dense<WT, ACT, true, true>(packed, T.hidden[0], obs_dim, x, h, lane);
#pragma unroll 1
  for (int l = 1; l < T.layers; ++l) {
    mlp_dense<WT, ACT, false, true>(packed, T.hidden[l], obs_dim, h, g, lane);
#pragma unroll
    for (int t = 0; t < WT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) h[t][i] = g[t][i];
  }
  if (T.head_dot) *row = mlp_dot<WT>(packed, T.head, h, lane);
  else mlp_dense<WT, ACT, false, false>(packed, T.head, obs_dim, h, out, lane);
}

// The four standard normals of one Philox4x32-10 block of the policy's stream (random.hpp: box_muller on words 0-1, 2-3).
__device__ __forceinline__ void mlp_normal4(unsigned env, unsigned call, unsigned block, unsigned k0, unsigned k1, float (&z)[4]) {
  unsigned r[4];
  philox4x32_10(env, call, 0u, ((unsigned)STREAM_POLICY << 24) | block, k0, k1, r);
  box_muller(r[0], r[1], z[0], z[1]);
  box_muller(r[2], r[3], z[2], z[3]);
}

template <int W, int ACT>
__global__ __launch_bounds__(128) void mlp_actor_critic_kernel(const MlpDev P, const float* __restrict__ packed, const float* __restrict__ obs,
                                                               const float* __restrict__ critic_obs, uint32_t* __restrict__ counters,
                                                               const MlpOutputs out) {
  constexpr int WT = W / 16;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4;
  const int env = blockIdx.x * 16 + (lane & 15);
  const bool valid = env < P.num_envs;
  if (wave == 0 ? !(P.run_actor || out.norm_obs) : !(P.run_critic || out.norm_critic_obs)) return;
  // this wave's input (wave-uniform): the actor's, or the critic's own row, width and statistics (the same for a symmetric shape)
  const bool actor_wave = __builtin_amdgcn_readfirstlane(wave) == 0;  // (scalar: the selections below stay in scalar registers)
  const float* __restrict__ in = actor_wave ? obs : critic_obs;
  const int in_dim = actor_wave ? P.obs_dim : P.critic_obs_dim;
  const int mean_off = actor_wave ? P.mean_off : P.critic_mean_off, std_off = actor_wave ? P.std_off : P.critic_std_off;
  float* __restrict__ norm_out = actor_wave ? out.norm_obs : out.norm_critic_obs;

  // observation (normalised): x[t][s] = element 16t + 4s + q of this lane's env, 0 past in_dim or num_envs
  float x[WT][4] = {};
  const int env_c = valid ? env : P.num_envs - 1;  // (loads clamped into the buffers and issued together; values past the batch discarded)
#pragma unroll
  for (int t = 0; t < WT; ++t) {
    if (16 * t < in_dim) {
      float v[4], m[4], sd[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = 16 * t + 4 * s + q, kc = k < in_dim ? k : in_dim - 1;
        v[s] = in[(size_t)env_c * in_dim + kc];
        m[s] = packed[mean_off + kc];
        sd[s] = packed[std_off + kc];
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = 16 * t + 4 * s + q;
        if (valid && k < in_dim) {
          float u = v[s];
          if (P.normalize) u = fminf(fmaxf((u - m[s]) / sd[s], -P.clip_obs), P.clip_obs);
          x[t][s] = u;
          if (norm_out) norm_out[(size_t)env * in_dim + k] = u;
        }
      }
    }
  }

  float head[WT][4] = {};
  if (wave == 1) {
    if (!P.run_critic) return;
    float v = 0.f;
    mlp_tower<WT, ACT>(packed, P.critic, in_dim, x, head, &v, lane);
    if (valid && q == 0) out.value[env] = v;
    return;
  }
  if (!P.run_actor) return;
  float m1 = 0.f;
  mlp_tower<WT, ACT>(packed, P.actor, P.obs_dim, x, head, &m1, lane);
  if (P.actor.head_dot) head[0][0] = m1;  // (action 0 is unit 0 of tile 0: lane group 0, accumulator 0)

  const unsigned call = valid && P.sample ? counters[env] : 0u;
  constexpr float HALF_LOG_2PI = 0.91893853320467274f;
  float lp = 0.f;
#pragma unroll
  for (int o = 0; o < (WT < 4 ? WT : 4); ++o) {
    const int a0 = 16 * o + 4 * q;
    if (o < P.act_tiles && a0 < P.act_dim) {
      float z[4] = {0.f, 0.f, 0.f, 0.f};
      if (P.sample) mlp_normal4((unsigned)env, call, (unsigned)(a0 >> 2), P.seed_lo, P.seed_hi, z);
      const mlp_f4 log_std = mlp_load4(packed + P.log_std_off + a0);
      const mlp_f4 low = mlp_load4(packed + P.low_off + a0), high = mlp_load4(packed + P.high_off + a0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int a = a0 + i;
        if (a < P.act_dim) {
          const float m = head[o][i], sigma = expf(log_std[i]);
          const float act = P.sample ? m + sigma * z[i] : m;
          const float d = act - m;
          lp += -(d * d) / (2.f * sigma * sigma) - log_std[i] - HALF_LOG_2PI;
          if (valid) {
            const size_t w = (size_t)env * P.act_dim + a;
            if (out.mean) out.mean[w] = m;
            if (out.action) out.action[w] = act;
            if (out.env_action) out.env_action[w] = fminf(fmaxf(act, low[i]), high[i]);
          }
        }
      }
    }
  }
  lp += __shfl_xor(lp, 16);
  lp += __shfl_xor(lp, 32);
  if (valid && q == 0) {
    if (out.log_prob) out.log_prob[env] = lp;
    if (P.sample) counters[env] = call + 1u;
  }
}

#endif  // __HIPCC__

}  // namespace upkie
