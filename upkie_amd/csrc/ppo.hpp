// ppo.hpp -- the learner half of PPO on the device: one minibatch of Stable-Baselines3's PPO.train (clipped surrogate,
// value loss, entropy bonus, their gradient through both MLP towers, clip_grad_norm_, Adam) on the packed weight buffer
// the rollout kernel reads (csrc/policy_mlp.hpp), in three launches per minibatch plus one per epoch. include/upkie_hip.h
// states the arithmetic; Python: upkie_amd/ppo.py.
//
// Launch 0, advantage statistics (once per epoch): block j reduces the advantages of minibatch j of the epoch's
// permutation in fp64 (two passes, a fixed LDS tree) into (mean, std + 1e-8), or (0, 1) without normalisation.
//
// Launch A, gradient. A block of NW waves (1-4, as many 16-sample tiles as fit the LDS budget) takes chunks of NW tiles
// of the minibatch in turn (chunk blockIdx.x, + gridDim.x, ...); wave w owns tile w of a chunk, lane l its sample l & 15,
// gathered through the permutation straight from the buffer's [T, N, ...] tensors. Per tower (actor, then critic):
//   forward: policy_mlp.hpp's mlp_dense / mlp_dot (transposed layers on v_mfma_f32_16x16x4_f32, lane = sample,
//     accumulators feeding the next layer), each layer's output also stored to the wave's LDS stage as [unit][sample];
//   loss: the sample's log-probability, ratio, clipped surrogate (or value loss) and their derivative dZ of the head;
//   backward, layer by layer from the head: dX = W^T dZ sums over the accumulator's row index, so it is one MFMA chain
//     with no lane movement (A = a W^T fragment gathered from the packed weights, B = the lane's own dZ accumulators);
//     dZ of the layer below = dX * act'(H), written over H in the stage. dW = dZ X^T sums over samples (the lane index):
//     after a barrier every wave reads the whole chunk's [unit][sample] stage transposed -- that is the one transpose
//     per layer -- and each 16 x 16 fragment of dW (owned by wave f % NW) is a chain of 4 NW MFMAs whose result lands in
//     the packed layout directly. Biases, dot heads and log_std are VALU sums over the stage's samples.
// The block's partial gradient (fp32, the packed layout from log_std_off on) lives in the workspace: its first chunk
// writes it, later chunks add to it (every word has one owning thread, so no atomics and no race). Loss sums (fp64,
// per lane, then a fixed shuffle tree and wave order) go to a per-block stats partial.
//
// Launch B, fold: thread i sums word i of the G partials in block order (+ the entropy term of log_std), writes the
// minibatch gradient and its square; a fixed LDS tree gives one sum of squares per block; the ticket (block_reduce.hpp)
// lets the last block form ||g||, the clip coefficient, the statistics row, t += 1 and Adam's bias corrections, all in
// a fixed order.
//
// Launch C, Adam: element-wise over the trainable words (log_std_off on; the fixed obs_mean / obs_std / action bounds
// before it are never written; padding words have a zero gradient, so m, v and the word stay 0).
//
// Data-parallel form (several ranks, each with its own samples; the result is one learner on the union): launch A
// scales by the global minibatch size (`count`, = mb_size in the fused form); launch B' (local fold) sums the G partials
// in block order into this rank's slot (train_words fp32 words, then PPO_STATS fp64 loss sums; no entropy term); the
// caller exchanges the slots so that every rank holds every rank's row, bit for bit; launch B then runs on the slots as
// its partials (W of them, in rank order) and adds the entropy term once; launch C is unchanged. The advantage
// statistics split the same way: per-minibatch sums (launch 0a, phase 0), exchange, squared deviations about the
// global mean (launch 0a, phase 1), exchange, (mean, std + 1e-8) over the global count (launch 0b). With one rank every
// output is the same bits as the fused form's.
//
// Asymmetric shape (critic_obs_dim = Dc > 0; PpoDev::critic_obs): the two towers read different rows of the same sample.
// The critic's stage has its own x region of tiles(Dc) rows of 16 (the actor's tiles(obs_dim)), and between the towers
// every wave restages x from critic_obs -- all 16 rows of each of its tiles(Dc) tiles, zeros past Dc, so nothing the actor
// left in the stage is read as critic input -- normalised with the critic's statistics unless obs_normalized. One more
// x load per sample per chunk; a symmetric shape takes no restage and computes word for word what it did.
//
// Every launch argument is constant for a given (epoch, minibatch) position: counters, t, lr and the permutation live
// in device memory, so the whole sequence can be captured in a hipGraph and replayed.
//
// Controlled form (PpoDev::ctrl != nullptr; the *_controlled entry points): the hyper-parameters that change during
// training and SB3's target_kl early stop live in a control block of PPO_CTRL_WORDS fp64 words (include/upkie_hip.h):
// launch A reads clip_range / clip_range_vf from it instead of its arguments; launch B's last block, after it wrote the
// statistics row, sets `stopped` when approx_kl > 1.5 target_kl and then neither advances t nor forms the step; once
// `stopped` is set every launch of the remaining minibatches returns at once (launch B writes a NaN statistics row),
// so the weights, m, v and t are those after the last minibatch that ran. The flag is written by one launch and read
// by later ones: stream order makes it visible, no fence is added. ppo_begin_kernel re-arms the block per update.
//
// Mirrored form (MIR = true; upkie_ppo_minibatch_update_mirror): every sample s of the minibatch has a mirrored partner --
// observation row M_o obs_s (word k = sign[k] * row[index[k]], gathered by ppo_stage_x BEFORE its normalisation, which then
// uses the statistics of word k), critic row M_c critic_obs_s, action M_a action_s, and the original's old log-prob, old
// value, return and normalised advantage. Original and partner are adjacent samples 2j, 2j + 1 of one 16-sample tile (lane
// parity r & 1 tells them apart; a tail never splits a pair), so the launch runs tiles(2 B) tiles through the same towers.
// The partner's PPO terms count only when `augment` (the loss means then run over n = 2 B positions); approx_kl and the
// clip fraction run over the originals alone. The mirror loss L_m = 1/(B A) sum (mu(M_o x_s)[a] - sign[a] mu(x_s)[index[a]])^2
// trains through the mirrored forward only: the tile's means go through the wave's own head rows of the stage, the mirrored
// lane reads its partner's unit index[a] there ([index[a]][r ^ 1]; a dot head with one action needs one shuffle) and adds
// mirror_coef 2 e / (B A) to its head dZ. A fifth fp64 loss sum collects e^2; the fold (ppo_fold<true>) writes 8 statistics
// words. MIR = false compiles to what the kernels were before the parameter.
//
// Explained variance (ppo_explained_variance_kernel): 1 - Var(returns - values) / Var(returns) over the T N samples,
// one block, the same two fp64 passes and LDS tree as launch 0.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/upkie_hip.h"
#include "block_reduce.hpp"
#include "policy_mlp.hpp"

namespace upkie {

enum {
  PPO_THREADS = 256,           // launches B, C
  PPO_ADV_THREADS = 1024,      // launch 0
  PPO_HEADER_BYTES = 256,      // ticket (u32 at 0), then coef, step size, sqrt(1 - beta2^t) as fp32 at words 4-6
  PPO_LDS_BUDGET = 65280,      // dynamic LDS of launch A when the stage of one tile fits (64 KiB less the static part)
  // the largest one-tile stage of any valid shape (obs 256, four 256-unit layers, act 64: 16 (256 + 4 * 256 + 64 + 64) floats)
  PPO_LDS_MAX = 4 * 16 * (256 + 4 * 256 + 64 + 64),
  PPO_MAX_GRID = 512,          // blocks of launch A
  PPO_STATS = 4,               // per-block loss sums: min(surrogates), (R - v_pred)^2, approx_kl terms, clipped count
  PPO_MIRROR_STATS = 5,        // the mirrored form's: those, then the mirror loss's squared errors
  // the control block's fp64 words (UPKIE_PPO_CTRL_* of include/upkie_hip.h); lr and t where adam_scalars has them
  PPO_CTRL_LR = 0,
  PPO_CTRL_T = 1,
  PPO_CTRL_CLIP_RANGE = 2,
  PPO_CTRL_CLIP_RANGE_VF = 3,  // 0: no value clipping
  PPO_CTRL_TARGET_KL = 4,      // 0: no early stop
  PPO_CTRL_STOPPED = 5,        // 0 / 1
  PPO_CTRL_N_UPDATES = 6,      // epochs entered since the block was zeroed (SB3's _n_updates)
  PPO_CTRL_MINIBATCHES_RUN = 7,  // statistics rows written by this update (the minibatch that stopped it included)
  PPO_CTRL_WORDS = 8,
};
static const int64_t PPO_PARTIAL_CAP_BYTES = 48ll << 20;  // partial gradients (the grid shrinks for large networks)

// LDS stage of one 16-sample tile for one tower, in rows of 16 floats: the input x (tiles(obs) rows of 16), each hidden
// layer's output H_l (later its dZ), the head's dZ (1 row for a dot head) and, for the actor, the per-sample log_std
// terms.
struct PpoStage {
  int h_off[UPKIE_MLP_MAX_LAYERS];  // float offsets (x at 0)
  int head_off, ls_off, floats;
};

struct PpoDev {
  MlpDev net;
  PpoStage stage[2];  // actor, critic
  int train_off, train_words;
  int mb_start, mb_size, nw, tile_floats, grid, fold_blocks;
  int count;                      // samples the loss means run over: mb_size, or the global minibatch size (all ranks)
  int part_stride, stat_stride;   // launch B: floats between two gradient partials, doubles between two loss-sum partials
  int obs_normalized, vf_clip;
  int asym;  // the critic reads critic_obs (restaged between the towers)
  float clip_lo, clip_hi, clip_range, clip_vf, ent_coef, vf_coef, max_grad_norm, beta1, beta2, adam_eps;
  const int32_t* perm;
  const float* obs;
  const float* critic_obs;  // [total][critic_obs_dim] when asym
  const float* actions;
  const float* old_values;
  const float* old_log_prob;
  const float* advantages;
  const float* returns;
  const double* adv_stats;  // this minibatch's (mean, denominator)
  float* packed;
  float* m;
  float* v;
  double* scalars;  // lr, t
  double* ctrl;     // the control block (scalars is its first two words), or nullptr: every value is a launch argument
  float* stats;     // [7]
  unsigned* ticket;
  float* header;
  float* partials;        // [grid][train_words]
  double* stat_partials;  // [grid][stat_stride]
  float* grad;            // [train_words]
  double* sq_partials;    // [fold_blocks]
  float* slot;            // launch B': this rank's slot (ppo_slot_words floats)
  // the mirrored form (MIR instantiations only; at the end, so that every other field stays where it was)
  int mir_augment;        // 0 / 1: the partners' PPO terms count
  float mirror_coef;
  const int32_t* mir_obs_index;  // the validated tables (ppo_mirror_words): word k of a mirrored row = sign[k] * row[index[k]]
  const float* mir_obs_sign;
  const int32_t* mir_critic_index;  // (the observation's for a symmetric shape: never read there)
  const float* mir_critic_sign;
  const int32_t* mir_act_index;
  const float* mir_act_sign;
};

struct PpoPlan {
  PpoStage stage[2];
  int train_off, train_words, nw, tile_floats, lds_bytes, grid_cap, fold_blocks;
};

__host__ __device__ inline int ppo_tiles(int n) { return (int)(((int64_t)n + 15) / 16); }  // (no overflow up to INT_MAX)

// Stage layout, waves per block, grid cap and workspace sizes of a shape; false for a shape out of range or without a
// critic.
inline bool ppo_plan(const UpkieMlpShape& s, PpoPlan* plan) {
  MlpDev d;
  const int64_t words = mlp_layout(s, &d);
  if (words < 0 || s.critic_layers < 1) return false;
  PpoPlan p{};
  auto stage = [&](const MlpTowerDev& T, bool actor) {
    PpoStage st{};
    int off = 16 * 16 * ppo_tiles(actor ? d.obs_dim : d.critic_obs_dim);  // (x: the tower's own input; the tile is sized by the larger stage)
    for (int l = 0; l < T.layers; ++l) st.h_off[l] = off, off += 16 * 16 * T.hidden[l].out_tiles;
    st.head_off = off, off += T.head_dot ? 16 : 16 * 16 * T.head.out_tiles;
    st.ls_off = off;
    if (actor) off += 16 * 16 * d.act_tiles;
    st.floats = off;
    return st;
  };
  p.stage[0] = stage(d.actor, true);
  p.stage[1] = stage(d.critic, false);
  p.tile_floats = p.stage[0].floats > p.stage[1].floats ? p.stage[0].floats : p.stage[1].floats;
  const int tile_bytes = 4 * p.tile_floats;
  p.nw = PPO_LDS_BUDGET / tile_bytes;
  p.nw = p.nw < 1 ? 1 : p.nw > 4 ? 4 : p.nw;
  p.lds_bytes = p.nw * tile_bytes;  // (<= PPO_LDS_MAX: a larger one tile is not possible)
  if (p.lds_bytes > PPO_LDS_MAX) return false;
  p.train_off = d.log_std_off;
  p.train_words = (int)(words - d.log_std_off);
  int64_t cap = PPO_PARTIAL_CAP_BYTES / (4 * (int64_t)p.train_words);
  p.grid_cap = cap < 1 ? 1 : cap > PPO_MAX_GRID ? PPO_MAX_GRID : (int)cap;
  p.fold_blocks = (p.train_words + PPO_THREADS - 1) / PPO_THREADS;
  if (plan) *plan = p;
  return true;
}

// Blocks of launch A for a minibatch of n samples.
inline int ppo_grid(const PpoPlan& p, int n) {
  const int chunks = (ppo_tiles(n) + p.nw - 1) / p.nw;
  return chunks < p.grid_cap ? chunks : p.grid_cap;
}

// Workspace offsets (bytes) for a grid of g blocks.
inline int64_t ppo_stat_partials_at(const PpoPlan& p, int g) { return PPO_HEADER_BYTES + 4 * (int64_t)g * p.train_words; }
inline int64_t ppo_grad_at(const PpoPlan& p, int g) { return ppo_stat_partials_at(p, g) + 8 * (int64_t)g * PPO_STATS; }
inline int64_t ppo_sq_at(const PpoPlan& p, int g) { return ppo_grad_at(p, g) + 4 * (int64_t)p.train_words; }
inline int64_t ppo_workspace_bytes(const PpoPlan& p, int g) { return ppo_sq_at(p, g) + 8 * (int64_t)p.fold_blocks; }

// A rank's slot of the data-parallel form: the gradient (train_words fp32, padded to an even count), then the PPO_STATS
// fp64 loss sums, in fp32 words (an even count: every slot of a [world][words] array stays 8-byte aligned).
inline int ppo_slot_stats_at(const PpoPlan& p) { return (p.train_words + 1) & ~1; }
inline int ppo_slot_words(const PpoPlan& p) { return ppo_slot_stats_at(p) + 2 * PPO_STATS; }

// The mirrored form: its table block (32-bit words: index then sign, for the observation, the critic's row of an
// asymmetric shape, and the action), the grid of a minibatch of n samples (2 n positions), and its workspace -- the plain
// layout with PPO_MIRROR_STATS loss sums per block.
inline int64_t ppo_mirror_words(const UpkieMlpShape& s) { return 2 * ((int64_t)s.obs_dim + s.critic_obs_dim + s.act_dim); }
inline int ppo_mirror_grid(const PpoPlan& p, int n) { return ppo_grid(p, 2 * n); }  // (n <= INT_MAX / 2: the entry points check)
inline int64_t ppo_mirror_grad_at(const PpoPlan& p, int g) { return ppo_stat_partials_at(p, g) + 8 * (int64_t)g * PPO_MIRROR_STATS; }
inline int64_t ppo_mirror_sq_at(const PpoPlan& p, int g) { return ppo_mirror_grad_at(p, g) + 4 * (int64_t)p.train_words; }
inline int64_t ppo_mirror_workspace_bytes(const PpoPlan& p, int g) { return ppo_mirror_sq_at(p, g) + 8 * (int64_t)p.fold_blocks; }

#if defined(__HIPCC__)

template <int ACT>
__device__ __forceinline__ float ppo_dact(float h) {  // the activation's derivative from its output
  if constexpr (ACT == UPKIE_MLP_TANH) return 1.f - h * h;
  else return h > 0.f ? 1.f : 0.f;
}

// dx = W^T dz for a layer in hidden (accumulator) k order: A = the W^T fragment W[16o + 4q + s][16t + r], gathered from
// packed word (o, t, lane 16 (r >> 2) + 4q + s, step r & 3); B = the lane's own accumulator s of dz tile o. dx tile t
// comes out in the accumulator layout of the layer's input (units 16t + 4q + i of sample r).
template <int WT>
__device__ __forceinline__ void ppo_dx(const float* __restrict__ packed, const MlpLayerDev& L, const float (&dz)[WT][4], float (&dx)[WT][4],
                                       int lane) {
  const int q = lane >> 4, r = lane & 15;
#pragma unroll
  for (int t = 0; t < WT; ++t) {
    mlp_f4 acc = {0.f, 0.f, 0.f, 0.f};
    if (t < L.in_tiles) {
#pragma unroll
      for (int o = 0; o < WT; ++o) {
        if (o < L.out_tiles) {
          const float* w = packed + L.w_off + ((o * L.in_tiles + t) * 64 + 16 * (r >> 2) + 4 * q) * 4 + (r & 3);
          float a[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) a[s] = w[4 * s];
#pragma unroll
          for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], dz[o][s], acc, 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) dx[t][i] = acc[i];
  }
}

// Partial-gradient word: the first chunk of a block writes it, later chunks add to it (same owning thread every chunk).
__device__ __forceinline__ void ppo_acc(float* part, int i, float x, bool first) { part[i] = first ? x : part[i] + x; }

// dW of an MFMA layer over the chunk's samples: fragment (o, t) = sum over samples of X[16t + r][k] dZ[16o + r'][k],
// read transposed from every wave's stage ([unit][sample] rows); A = X^T, B = dZ^T, k = 4 samples per step, so lane
// (q, r) ends with W[16o + r][16t + 4q + i], packed word (o, t, lane, i) -- or, for the first layer (natural k order),
// (o, t, lane 16i + r, step q). Then the bias: the sum of dZ's rows.
__device__ __forceinline__ void ppo_dw_mfma(const PpoDev& P, const float* stage, const MlpLayerDev& L, bool first_layer, int x_off, int z_off,
                                            float* part, bool first, int wave, int lane) {
  const int q = lane >> 4, r = lane & 15;
  const int frags = L.out_tiles * L.in_tiles;
  for (int f = wave; f < frags; f += P.nw) {
    const int o = f / L.in_tiles, t = f - o * L.in_tiles;
    mlp_f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < P.nw; ++w) {
      const float* tb = stage + w * P.tile_floats;
      const float* xa = tb + x_off + (16 * t + r) * 16 + q;
      const float* zb = tb + z_off + (16 * o + r) * 16 + q;
      float a[4], b[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) a[s] = xa[4 * s], b[s] = zb[4 * s];
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
    }
    const int base = L.w_off - P.train_off + (o * L.in_tiles + t) * 256;
#pragma unroll
    for (int i = 0; i < 4; ++i) ppo_acc(part, base + (first_layer ? (16 * i + r) * 4 + q : lane * 4 + i), acc[i], first);
  }
  const int tid = wave * 64 + lane;
  for (int u = tid; u < 16 * L.out_tiles; u += 64 * P.nw) {
    float s = 0.f;
    for (int w = 0; w < P.nw; ++w) {
      const float* z = stage + w * P.tile_floats + z_off + u * 16;
#pragma unroll
      for (int k = 0; k < 16; ++k) s += z[k];
    }
    ppo_acc(part, L.b_off - P.train_off + u, s, first);
  }
}

// dW of a dot head (one row dz at z_off): word k = sum over samples of dz X[k]; bias word = sum of dz (its 3 padding
// words 0).
__device__ __forceinline__ void ppo_dw_dot(const PpoDev& P, const float* stage, const MlpLayerDev& L, int x_off, int z_off, float* part, bool first,
                                           int tid) {
  for (int k = tid; k < 16 * L.in_tiles + 4; k += 64 * P.nw) {
    float s = 0.f;
    if (k < 16 * L.in_tiles) {
      for (int w = 0; w < P.nw; ++w) {
        const float* tb = stage + w * P.tile_floats;
#pragma unroll
        for (int j = 0; j < 16; ++j) s = fmaf(tb[z_off + j], tb[x_off + k * 16 + j], s);
      }
      ppo_acc(part, L.w_off - P.train_off + k, s, first);
    } else {
      if (k == 16 * L.in_tiles)
        for (int w = 0; w < P.nw; ++w) {
          const float* tb = stage + w * P.tile_floats;
#pragma unroll
          for (int j = 0; j < 16; ++j) s += tb[z_off + j];
        }
      ppo_acc(part, L.b_off - P.train_off + (k - 16 * L.in_tiles), s, first);
    }
  }
}

// Sum over the chunk's samples of `rows` stage rows at `off` into partial words [at, at + rows).
__device__ __forceinline__ void ppo_row_sums(const PpoDev& P, const float* stage, int off, int rows, int at, float* part, bool first, int tid) {
  for (int u = tid; u < rows; u += 64 * P.nw) {
    float s = 0.f;
    for (int w = 0; w < P.nw; ++w) {
      const float* z = stage + w * P.tile_floats + off + u * 16;
#pragma unroll
      for (int k = 0; k < 16; ++k) s += z[k];
    }
    ppo_acc(part, at + u, s, first);
  }
}

// Writes accumulator tiles [0, tiles) of `h` as [unit][sample] rows at `off` of the wave's stage.
template <int WT>
__device__ __forceinline__ void ppo_store(float* my, int off, int tiles, const float (&h)[WT][4], int lane) {
  const int q = lane >> 4, r = lane & 15;
#pragma unroll
  for (int t = 0; t < WT; ++t)
    if (t < tiles)
#pragma unroll
      for (int i = 0; i < 4; ++i) my[off + (16 * t + 4 * q + i) * 16 + r] = h[t][i];
}

// The clipping constants of launch A: its arguments, or (controlled form) the control block's words.
struct PpoClip {
  float lo, hi, range, vf;
  int vf_on;
};

__device__ __forceinline__ float ppo_uniform(float x) {  // (a value every lane holds: keep it in a scalar register)
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}

// One tower of one chunk: forward, loss, backward, dW. ACTOR: the policy loss through the Gaussian head (and log_std);
// otherwise the value loss through the critic's dot head. `st` collects the loss sums of the lane's sample (lanes of
// group 0 only). BC (distill.hpp; ACTOR only): the behaviour-cloning head instead of the surrogate -- the labels are read
// where the actions are, dZ = 2 (mean - label) / (count A), st[0] collects every lane's own (mean - label)^2, and
// log_std gets no stage rows and no partial words. BC = false compiles to what it did before the parameter.
// MIR (the mirrored form, not with BC): odd samples of the tile are the mirrored partners of the even ones -- their action is
// M_a action, their PPO terms count only under `augment` (`live`), the means run over n positions, the KL and clip sums skip
// them, and the actor adds the mirror loss's dZ to theirs and its squared errors to st[4]. MIR = false likewise.
template <int WT, int ACT, bool ACTOR, bool BC = false, bool MIR = false>
__device__ __forceinline__ void ppo_tower(const PpoDev& P, const PpoClip& K, float* stage, int sample, bool valid, float* part, bool first,
                                          double (&st)[MIR ? PPO_MIRROR_STATS : PPO_STATS], int wave, int lane) {
  const int q = lane >> 4, r = lane & 15, tid = wave * 64 + lane;
  const MlpTowerDev& T = ACTOR ? P.net.actor : P.net.critic;
  const PpoStage& S = P.stage[ACTOR ? 0 : 1];
  const int in_dim = ACTOR ? P.net.obs_dim : P.net.critic_obs_dim;  // (the tower's input width)
  const float* __restrict__ packed = P.packed;
  float* my = stage + wave * P.tile_floats;
  const float inv_b = MIR ? 1.f / ((float)P.count * (float)(1 + P.mir_augment)) : 1.f / (float)P.count;
  const bool mir = MIR && (r & 1);                             // (a mirrored partner)
  const bool live = MIR ? valid && (!mir || P.mir_augment) : valid;  // (its PPO terms count)
  float cur[WT][4] = {};  // dZ of the current layer (accumulator layout)
  float dz_dot = 0.f;     // dZ of a dot head (every lane of the sample)
  {
    float x[WT][4] = {}, h[WT][4] = {};
    __syncthreads();  // (every wave is done reading the previous tower's stage)
#pragma unroll
    for (int t = 0; t < WT; ++t)
      if (16 * t < in_dim)
#pragma unroll
        for (int s = 0; s < 4; ++s) x[t][s] = my[(16 * t + 4 * s + q) * 16 + r];
    mlp_dense<WT, ACT, true, true>(packed, T.hidden[0], in_dim, x, h, lane);
    ppo_store<WT>(my, S.h_off[0], T.hidden[0].out_tiles, h, lane);
#pragma unroll 1
    for (int l = 1; l < T.layers; ++l) {
      mlp_dense<WT, ACT, false, true>(packed, T.hidden[l], in_dim, h, x, lane);
#pragma unroll
      for (int t = 0; t < WT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) h[t][i] = x[t][i];
      ppo_store<WT>(my, S.h_off[l], T.hidden[l].out_tiles, h, lane);
    }
    if constexpr (ACTOR) {
      float head[WT][4] = {};
      float m1 = 0.f;
      if (T.head_dot) m1 = mlp_dot<WT>(packed, T.head, h, lane);
      else mlp_dense<WT, ACT, false, false>(packed, T.head, in_dim, h, head, lane);
      if (T.head_dot) head[0][0] = m1;
      if constexpr (BC) {
        const float inv_ba = 1.f / ((float)P.count * (float)P.net.act_dim);
#pragma unroll
        for (int o = 0; o < (WT < 4 ? WT : 4); ++o) {
          if (o < P.net.act_tiles) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int a = 16 * o + 4 * q + i;
              float dz = 0.f;
              if (valid && a < P.net.act_dim) {
                const float e = head[o][i] - P.actions[(size_t)sample * P.net.act_dim + a];  // (the label)
                st[0] += (double)e * (double)e;
                dz = 2.f * e * inv_ba;
              }
              cur[o][i] = dz;
            }
          }
        }
      } else {
        if constexpr (MIR) {
          // the mirror loss: e = mu(M_o x)[a] - sign[a] mu(x)[index[a]] on the mirrored lanes, the partner's means read from
          // the wave's own head rows ([unit][sample]); its dZ waits in `cur` for the surrogate's
          float partner = 0.f;
          if (T.head_dot) {
            partner = __shfl_xor(m1, 1);
          } else {
            ppo_store<WT>(my, S.head_off, T.head.out_tiles, head, lane);
            __syncthreads();
          }
          const float c = 2.f * P.mirror_coef / ((float)P.count * (float)P.net.act_dim);
#pragma unroll
          for (int o = 0; o < (WT < 4 ? WT : 4); ++o) {
            if (o < P.net.act_tiles) {
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int a = 16 * o + 4 * q + i;
                if (mir && valid && a < P.net.act_dim) {
                  const float target = T.head_dot ? partner : my[S.head_off + P.mir_act_index[a] * 16 + (r ^ 1)];
                  const float e = head[o][i] - P.mir_act_sign[a] * target;
                  st[4] += (double)e * (double)e;
                  cur[o][i] = c * e;
                }
              }
            }
          }
          if (!T.head_dot) __syncthreads();  // (the means are read: the head's dZ goes over them)
        }
        constexpr float HALF_LOG_2PI = 0.91893853320467274f;
        float lp = 0.f, d[4][4] = {}, sig2[4][4] = {};
#pragma unroll
        for (int o = 0; o < (WT < 4 ? WT : 4); ++o) {
          const int a0 = 16 * o + 4 * q;
          if (o < P.net.act_tiles && a0 < P.net.act_dim) {
            const mlp_f4 log_std = mlp_load4(packed + P.net.log_std_off + a0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int a = a0 + i;
              if (a < P.net.act_dim) {
                const float sigma = expf(log_std[i]);
                float action = P.actions[(size_t)sample * P.net.act_dim + a];
                if constexpr (MIR)
                  if (mir) action = P.mir_act_sign[a] * P.actions[(size_t)sample * P.net.act_dim + P.mir_act_index[a]];
                const float dd = action - head[o][i];
                d[o][i] = dd, sig2[o][i] = sigma * sigma;
                lp += -(dd * dd) / (2.f * sigma * sigma) - log_std[i] - HALF_LOG_2PI;
              }
            }
          }
        }
        lp += __shfl_xor(lp, 16);
        lp += __shfl_xor(lp, 32);
        // clipped surrogate: d loss / d log_prob (torch.minimum splits a tie half / half; clamp passes at its bounds)
        const double* as = P.adv_stats;
        const float adv = (float)(((double)P.advantages[sample] - as[0]) / as[1]);
        const float log_ratio = lp - P.old_log_prob[sample];
        const float ratio = expf(log_ratio);
        const float a1 = adv * ratio, a2 = adv * fminf(fmaxf(ratio, K.lo), K.hi);
        const float w1 = a1 < a2 ? 1.f : a1 == a2 ? 0.5f : 0.f, w2 = 1.f - w1;
        const float pass = ratio >= K.lo && ratio <= K.hi ? 1.f : 0.f;
        const float g_lp = live ? -inv_b * (w1 * adv + w2 * adv * pass) * ratio : 0.f;
        if (live && q == 0) st[0] += (double)fminf(a1, a2);
        if (valid && !mir && q == 0) {
          st[2] += (double)((ratio - 1.f) - log_ratio);
          st[3] += fabsf(ratio - 1.f) > K.range ? 1.0 : 0.0;
        }
        // head dZ = d loss / d mean, and the per-sample log_std terms, into the stage
#pragma unroll
        for (int o = 0; o < (WT < 4 ? WT : 4); ++o) {
          if (o < P.net.act_tiles) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const bool on = 16 * o + 4 * q + i < P.net.act_dim;
              const float dmu = on ? g_lp * d[o][i] / sig2[o][i] : 0.f;
              cur[o][i] = MIR ? cur[o][i] + dmu : dmu;
              my[S.ls_off + (16 * o + 4 * q + i) * 16 + r] = on ? g_lp * (d[o][i] * d[o][i] / sig2[o][i] - 1.f) : 0.f;
            }
          }
        }
      }
      if (T.head_dot) {
        dz_dot = __shfl(cur[0][0], r);  // (action 0: lane group 0, accumulator 0)
        if (q == 0) my[S.head_off + r] = dz_dot;
      } else {
        ppo_store<WT>(my, S.head_off, T.head.out_tiles, cur, lane);  // (tiles past act_tiles: zeros)
      }
    } else {
      const float v = mlp_dot<WT>(packed, T.head, h, lane);
      const float old_v = P.old_values[sample], ret = P.returns[sample];
      float vp = v, pass = 1.f;
      if (K.vf_on) {
        const float dv = v - old_v;
        vp = old_v + fminf(fmaxf(dv, -K.vf), K.vf);
        pass = dv >= -K.vf && dv <= K.vf ? 1.f : 0.f;
      }
      const float e = ret - vp;
      dz_dot = live ? P.vf_coef * 2.f * (vp - ret) * inv_b * pass : 0.f;
      if (live && q == 0) st[1] += (double)e * (double)e;
      if (q == 0) my[S.head_off + r] = dz_dot;
    }
  }

  // backward: layer l + 1 (the head when l = layers - 1) -> dZ of hidden layer l, over H_l in the stage
#pragma unroll 1
  for (int l = T.layers - 1; l >= 0; --l) {
    const bool head = l == T.layers - 1;
    const MlpLayerDev& U = head ? T.head : T.hidden[l + 1];
    const int z_off = head ? S.head_off : S.h_off[l + 1];
    __syncthreads();  // (dZ of layer l + 1 and H_l of every wave are in the stage)
    if (head && T.head_dot) ppo_dw_dot(P, stage, U, S.h_off[l], z_off, part, first, tid);
    else ppo_dw_mfma(P, stage, U, false, S.h_off[l], z_off, part, first, wave, lane);
    __syncthreads();  // (H_l read: it may be overwritten)
    float dx[WT][4] = {};
    if (head && T.head_dot) {
#pragma unroll
      for (int t = 0; t < WT; ++t)
        if (t < U.in_tiles) {
          const mlp_f4 w = mlp_load4(packed + U.w_off + 16 * t + 4 * q);
#pragma unroll
          for (int i = 0; i < 4; ++i) dx[t][i] = w[i] * dz_dot;
        }
    } else {
      ppo_dx<WT>(packed, U, cur, dx, lane);
    }
    const int tiles = T.hidden[l].out_tiles, off = S.h_off[l];
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      if (t < tiles) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int at = off + (16 * t + 4 * q + i) * 16 + r;
          const float dz = t < U.in_tiles ? dx[t][i] * ppo_dact<ACT>(my[at]) : 0.f;
          cur[t][i] = dz;
          my[at] = dz;
        }
      }
    }
  }
  __syncthreads();
  ppo_dw_mfma(P, stage, T.hidden[0], true, 0, S.h_off[0], part, first, wave, lane);
  if constexpr (ACTOR && !BC) ppo_row_sums(P, stage, S.ls_off, 16 * P.net.act_tiles, P.net.log_std_off - P.train_off, part, first, tid);
}

// The x rows of the wave's tile from `src` [total][dim]: element k of the sample, normalised as act() does (statistics at
// mean_off / std_off) unless the buffer holds normalised observations; all 16 rows of every tile below dim, zeros past it.
// MIR: a mirrored partner's (odd r) element k is sign[k] * row[index[k]], then normalised as word k. MIR = false compiles to
// what it did before the parameter.
template <int WT, bool MIR = false>
__device__ __forceinline__ void ppo_stage_x(const PpoDev& P, float* my, const float* __restrict__ src, int dim, int mean_off, int std_off, int sample,
                                            int q, int r, const int32_t* __restrict__ index = nullptr, const float* __restrict__ sign = nullptr) {
#pragma unroll
  for (int t = 0; t < WT; ++t) {
    if (16 * t < dim) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = 16 * t + 4 * s + q;
        float u = 0.f;
        if (k < dim) {
          u = src[(size_t)sample * dim + k];
          if constexpr (MIR)
            if (r & 1) u = sign[k] * src[(size_t)sample * dim + index[k]];
          if (P.net.normalize && !P.obs_normalized)
            u = fminf(fmaxf((u - P.packed[mean_off + k]) / P.packed[std_off + k], -P.net.clip_obs), P.net.clip_obs);
        }
        my[k * 16 + r] = u;
      }
    }
  }
}

// BC (distill.hpp): the actor tower alone under the behaviour-cloning head; the partials then span the actor's words
// (train_off = the actor's first weight word), so no log_std word and no critic word is written or folded.
// MIR: the mirrored form -- position j of the 2 mb_size is sample j >> 1, mirrored when j is odd -- with PPO_MIRROR_STATS sums.
template <int W, int ACT, bool BC = false, bool MIR = false>
__global__ __launch_bounds__(256) void ppo_grad_kernel(const PpoDev P) {
  static_assert(!(BC && MIR), "the behaviour-cloning head has no mirrored form");
  constexpr int NS = MIR ? PPO_MIRROR_STATS : PPO_STATS;
  extern __shared__ float stage[];
  __shared__ double red[4][NS];
  constexpr int WT = W / 16;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  float* part = P.partials + (size_t)blockIdx.x * P.train_words;
  float* my = stage + wave * P.tile_floats;
  double st[NS] = {};
  PpoClip K = {P.clip_lo, P.clip_hi, P.clip_range, P.clip_vf, P.vf_clip};
  if (P.ctrl) {  // (uniform over the grid: one scalar load; the clip constants as ppo_fill forms them from the config)
    if (P.ctrl[PPO_CTRL_STOPPED] != 0.0) return;
    const float cr = (float)P.ctrl[PPO_CTRL_CLIP_RANGE], cv = (float)P.ctrl[PPO_CTRL_CLIP_RANGE_VF];
    K.range = ppo_uniform(cr), K.lo = ppo_uniform((float)(1.0 - (double)cr)), K.hi = ppo_uniform((float)(1.0 + (double)cr));
    K.vf = ppo_uniform(cv), K.vf_on = K.vf > 0.f;
  }
  const int chunks = (ppo_tiles(MIR ? 2 * P.mb_size : P.mb_size) + P.nw - 1) / P.nw;
  for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
    const bool first = c == (int)blockIdx.x;
    const int64_t at = ((int64_t)c * P.nw + wave) * 16 + r;  // position in the minibatch (64-bit: no overflow near INT_MAX)
    const int64_t j = MIR ? at >> 1 : at;                    // (MIR: positions 2j, 2j + 1 are sample j and its partner)
    const bool valid = j < P.mb_size;
    const int sample = P.perm[(int64_t)P.mb_start + (valid ? j : 0)];
    __syncthreads();  // (the previous chunk's critic is done reading x)
    ppo_stage_x<WT, MIR>(P, my, P.obs, P.net.obs_dim, P.net.mean_off, P.net.std_off, sample, q, r, P.mir_obs_index, P.mir_obs_sign);
    ppo_tower<WT, ACT, true, BC, MIR>(P, K, stage, sample, valid, part, first, st, wave, lane);
    if constexpr (BC) continue;
    if (P.asym) {
      __syncthreads();  // (every wave is done reading the actor's x: its first-layer dW reads every wave's rows)
      ppo_stage_x<WT, MIR>(P, my, P.critic_obs, P.net.critic_obs_dim, P.net.critic_mean_off, P.net.critic_std_off, sample, q, r, P.mir_critic_index,
                           P.mir_critic_sign);
    }
    ppo_tower<WT, ACT, false, false, MIR>(P, K, stage, sample, valid, part, first, st, wave, lane);
  }
  // loss sums: a fixed shuffle tree per wave, then the waves in order
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    double x = st[k];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m);
    if (lane == 0) red[wave][k] = x;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    double s = 0.0;
    for (int w = 0; w < P.nw; ++w) s += red[w][threadIdx.x];
    P.stat_partials[blockIdx.x * NS + threadIdx.x] = s;
  }
}

// Launch B: fold the partials, ||g||^2 per block, and the last block's scalars (see the top of the file). MIR: the
// mirrored form's PPO_MIRROR_STATS sums and 8 statistics words; MIR = false is the kernel as it was.
template <bool MIR>
__device__ __forceinline__ void ppo_fold(const PpoDev& P) {
  constexpr int NS = MIR ? PPO_MIRROR_STATS : PPO_STATS;
  __shared__ double lds[PPO_THREADS + 1];
  const int tid = threadIdx.x, i = blockIdx.x * PPO_THREADS + tid;
  if (P.ctrl && P.ctrl[PPO_CTRL_STOPPED] != 0.0) {  // (read before any block's ticket, written after the last: no race)
    if (blockIdx.x == 0 && tid < (MIR ? 8 : 7)) P.stats[tid] = __builtin_nanf("");
    return;
  }
  double sq = 0.0;
  if (i < P.train_words) {
    float s = fold_in_block_order(P.partials + i, P.grid, P.part_stride);
    if (i < P.net.act_dim) s -= P.ent_coef;  // d(ent_coef * entropy_loss) / d log_std_a
    P.grad[i] = s;
    sq = (double)s * (double)s;
  }
  lds[tid] = sq;
  lds_tree_sum<PPO_THREADS>(tid, lds);
  if (tid == 0) P.sq_partials[blockIdx.x] = lds[0];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid != 0 || !ticket_draw(P.ticket, P.fold_blocks)) return;  // (block_reduce.hpp; thread 0 of the last block goes on alone)
  __hip_atomic_store(P.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  double total = 0.0;
  for (int b = 0; b < P.fold_blocks; ++b) total += P.sq_partials[b];
  const double norm = sqrt(total);
  const double coef = fmin(1.0, (double)P.max_grad_norm / (norm + 1e-6));
  double sums[NS] = {};
  for (int b = 0; b < P.grid; ++b)
#pragma unroll
    for (int k = 0; k < NS; ++k) sums[k] += P.stat_partials[(size_t)b * P.stat_stride + k];
  const double originals = (double)P.count;
  const double n = MIR ? originals * (double)(1 + P.mir_augment) : originals;  // (the positions the loss means run over)
  double entropy = 0.0;
  for (int a = 0; a < P.net.act_dim; ++a) entropy += 0.5 + 0.91893853320467274 + (double)P.packed[P.net.log_std_off + a];
  const double pg = -sums[0] / n, vl = sums[1] / n, ent_loss = -entropy;
  P.stats[0] = (float)pg;
  P.stats[1] = (float)vl;
  P.stats[2] = (float)ent_loss;
  if constexpr (MIR) {
    const double lm = sums[4] / (originals * (double)P.net.act_dim);
    P.stats[3] = (float)(pg + (double)P.ent_coef * ent_loss + (double)P.vf_coef * vl + (double)P.mirror_coef * lm);
    P.stats[7] = (float)lm;
  } else {
    P.stats[3] = (float)(pg + (double)P.ent_coef * ent_loss + (double)P.vf_coef * vl);
  }
  const float approx_kl = (float)(sums[2] / originals);
  P.stats[4] = approx_kl;
  P.stats[5] = (float)(sums[3] / originals);
  P.stats[6] = (float)norm;
  if (P.ctrl) {
    // SB3: n_updates counts the epochs entered; the losses are logged, then approx_kl (a float32) is held to 1.5 target_kl
    // and the update ends BEFORE this minibatch's optimiser step
    if (P.mb_start == 0) P.ctrl[PPO_CTRL_N_UPDATES] += 1.0;
    P.ctrl[PPO_CTRL_MINIBATCHES_RUN] += 1.0;
    const double target_kl = P.ctrl[PPO_CTRL_TARGET_KL];
    if (target_kl > 0.0 && (double)approx_kl > 1.5 * target_kl) {
      P.ctrl[PPO_CTRL_STOPPED] = 1.0;
      return;
    }
  }
  const double t = P.scalars[1] + 1.0;
  P.scalars[1] = t;
  P.header[4] = (float)coef;
  P.header[5] = (float)(P.scalars[0] / (1.0 - pow((double)P.beta1, t)));
  P.header[6] = (float)sqrt(1.0 - pow((double)P.beta2, t));
}

__global__ __launch_bounds__(PPO_THREADS) void ppo_fold_kernel(const PpoDev P) { ppo_fold<false>(P); }
__global__ __launch_bounds__(PPO_THREADS) void ppo_mirror_fold_kernel(const PpoDev P) { ppo_fold<true>(P); }

// Launch B' (data-parallel form): word i of this rank's slot = the sum of word i of the G partials in block order, as
// launch B sums them but without the entropy term; block 0 also sums the loss-sum partials in block order and zeroes the
// padding word. No ticket: launch B runs on the exchanged slots.
__global__ __launch_bounds__(PPO_THREADS) void ppo_local_fold_kernel(const PpoDev P) {
  const int tid = threadIdx.x, i = blockIdx.x * PPO_THREADS + tid;
  if (P.ctrl && P.ctrl[PPO_CTRL_STOPPED] != 0.0) return;  // (the slot keeps its last contents: launch B ignores them)
  if (i < P.train_words) P.slot[i] = fold_in_block_order(P.partials + i, P.grid, P.part_stride);
  if (blockIdx.x != 0) return;
  const int at = (P.train_words + 1) & ~1;
  if (tid < PPO_STATS) {
    double s = 0.0;
    for (int b = 0; b < P.grid; ++b) s += P.stat_partials[(size_t)b * P.stat_stride + tid];
    ((double*)(P.slot + at))[tid] = s;
  }
  if (tid == PPO_STATS && at != P.train_words) P.slot[P.train_words] = 0.f;
}

// Launch C: clip + Adam on the trainable words, in place.
__global__ __launch_bounds__(PPO_THREADS) void ppo_adam_kernel(const PpoDev P) {
  const int i = blockIdx.x * PPO_THREADS + threadIdx.x;
  if (i >= P.train_words) return;
  if (P.ctrl && P.ctrl[PPO_CTRL_STOPPED] != 0.0) return;  // (set by this minibatch's launch B, or an earlier one)
  const float coef = P.header[4], step = P.header[5], bc2 = P.header[6];
  const int w = P.train_off + i;
  const float g = P.grad[i] * coef;
  const float m = P.beta1 * P.m[w] + (1.f - P.beta1) * g;
  const float v = P.beta2 * P.v[w] + (1.f - P.beta2) * g * g;
  P.m[w] = m;
  P.v[w] = v;
  P.packed[w] -= step * (m / (sqrtf(v) / bc2 + P.adam_eps));
}

// One pass of launch 0 over minibatch `start`'s n advantages: the sum of x (or of (x - mean)^2 when `square`), each
// thread 8 gathers in flight at a time, then a fixed LDS tree. Every thread of the block calls it and gets the sum.
__device__ __forceinline__ double ppo_adv_pass(double* lds, int n, int start, const int32_t* __restrict__ perm, const float* __restrict__ adv,
                                               bool square, double mean) {
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int64_t i0 = tid; i0 < n; i0 += 8 * PPO_ADV_THREADS) {  // (64-bit: no overflow near INT_MAX)
    double x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t i = i0 + k * PPO_ADV_THREADS;
      x[k] = i < n ? (double)adv[perm[start + i]] - (square ? mean : 0.0) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s += square ? x[k] * x[k] : x[k];
  }
  lds[tid] = s;
  lds_tree_sum<PPO_ADV_THREADS>(tid, lds);
  const double r = lds[0];
  __syncthreads();
  return r;
}

// Launch 0: (mean, std + 1e-8) of the advantages of every minibatch of an epoch, fp64, two passes in a fixed order.
__global__ __launch_bounds__(PPO_ADV_THREADS) void ppo_adv_stats_kernel(int total, int batch, const int32_t* __restrict__ perm,
                                                                       const float* __restrict__ adv, int normalize, double* __restrict__ out) {
  __shared__ double lds[PPO_ADV_THREADS];
  const int start = blockIdx.x * batch;
  const int n = total - start < batch ? total - start : batch;
  if (!normalize || n < 2) {
    if (threadIdx.x == 0) out[2 * blockIdx.x] = 0.0, out[2 * blockIdx.x + 1] = 1.0;
    return;
  }
  const double mean = ppo_adv_pass(lds, n, start, perm, adv, false, 0.0) / n;
  const double var = ppo_adv_pass(lds, n, start, perm, adv, true, mean) / (n - 1);
  if (threadIdx.x == 0) out[2 * blockIdx.x] = mean, out[2 * blockIdx.x + 1] = sqrt(var) + 1e-8;
}

// Launch 0a (data-parallel form), block j = minibatch j of M: phase 0 writes its local sum to mine[j]; phase 1 (after
// the exchange) forms the global mean from slots[r][j], r in rank order, over world * n samples (every rank holds n),
// and writes the local sum of squared deviations about it to mine[M + j]. mine / slots[r]: 2 M doubles.
__global__ __launch_bounds__(PPO_ADV_THREADS) void ppo_adv_partials_kernel(int total, int batch, const int32_t* __restrict__ perm,
                                                                          const float* __restrict__ adv, int phase, const double* __restrict__ slots,
                                                                          int world, double* __restrict__ mine) {
  __shared__ double lds[PPO_ADV_THREADS];
  const int j = blockIdx.x, M = gridDim.x, start = j * batch;
  const int n = total - start < batch ? total - start : batch;
  if (phase == 0) {
    const double s = ppo_adv_pass(lds, n, start, perm, adv, false, 0.0);
    if (threadIdx.x == 0) mine[j] = s;
    return;
  }
  double g = slots[j];
  for (int r = 1; r < world; ++r) g += slots[(size_t)r * 2 * M + j];
  const double mean = g / ((double)world * n);
  const double q = ppo_adv_pass(lds, n, start, perm, adv, true, mean);
  if (threadIdx.x == 0) mine[M + j] = q;
}

// Launch 0b (data-parallel form): out[j] = (mean, std + 1e-8) over the world * n samples of minibatch j from the
// exchanged slots (sums in rank order; std unbiased), or (0, 1) when normalize is 0 or there is one sample.
__global__ __launch_bounds__(PPO_THREADS) void ppo_adv_finish_kernel(int total, int batch, int minibatches, int normalize, const double* __restrict__ slots,
                                                                    int world, double* __restrict__ out) {
  const int j = blockIdx.x * PPO_THREADS + threadIdx.x, M = minibatches;
  if (j >= M) return;
  const int start = j * batch;
  const int n = total - start < batch ? total - start : batch;
  const double cnt = (double)world * n;
  if (!normalize || cnt < 2.0) {
    out[2 * j] = 0.0, out[2 * j + 1] = 1.0;
    return;
  }
  double g = slots[j], q = slots[M + j];
  for (int r = 1; r < world; ++r) g += slots[(size_t)r * 2 * M + j], q += slots[(size_t)r * 2 * M + M + j];
  const double mean = g / cnt;
  out[2 * j] = mean, out[2 * j + 1] = sqrt(q / (cnt - 1.0)) + 1e-8;
}

// Re-arms a control block at the start of an update: the early stop of the previous update is over.
__global__ void ppo_begin_kernel(double* ctrl) {
  if (threadIdx.x == 0) ctrl[PPO_CTRL_STOPPED] = 0.0, ctrl[PPO_CTRL_MINIBATCHES_RUN] = 0.0;
}

// Writes the host-set words of a control block (upkie_ppo_control_set).
__global__ void ppo_control_set_kernel(double* ctrl, double lr, double clip_range, double clip_range_vf, double target_kl) {
  if (threadIdx.x != 0) return;
  ctrl[PPO_CTRL_LR] = lr, ctrl[PPO_CTRL_CLIP_RANGE] = clip_range;
  ctrl[PPO_CTRL_CLIP_RANGE_VF] = clip_range_vf, ctrl[PPO_CTRL_TARGET_KL] = target_kl;
}

// One pass of the explained variance over the n samples: (sum of y, sum of d) with y = returns, d = returns - values,
// or of their squared deviations about (mean_y, mean_d) when `square`; ppo_adv_pass's order: 8 loads in flight per
// thread, then a fixed LDS tree per sum. Every thread of the block calls it and gets both sums.
__device__ __forceinline__ void ppo_ev_pass(double (*lds)[PPO_ADV_THREADS], int n, const float* __restrict__ ret, const float* __restrict__ val,
                                            bool square, double mean_y, double mean_d, double* sum_y, double* sum_d) {
  const int tid = threadIdx.x;
  double sy = 0.0, sd = 0.0;
  for (int64_t i0 = tid; i0 < n; i0 += 8 * PPO_ADV_THREADS) {
    double y[8], d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t i = i0 + k * PPO_ADV_THREADS;
      const bool in = i < n;
      const double r = in ? (double)ret[i] : 0.0, v = in ? (double)val[i] : 0.0;
      y[k] = in ? r - (square ? mean_y : 0.0) : 0.0;
      d[k] = in ? (r - v) - (square ? mean_d : 0.0) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) sy += square ? y[k] * y[k] : y[k], sd += square ? d[k] * d[k] : d[k];
  }
  lds[0][tid] = sy, lds[1][tid] = sd;
  lds_tree_sum<PPO_ADV_THREADS>(tid, lds[0], lds[1]);
  *sum_y = lds[0][0], *sum_d = lds[1][0];
  __syncthreads();
}

// Explained variance of the critic (SB3's explained_variance(values, returns): population variances, NaN when
// Var(returns) == 0), one block. phase < 0: everything on this rank's n samples, out[0] = the result. Data-parallel form
// (every rank n samples, slots[r] = rank r's 4 doubles): phase 0 writes the local sums to mine[0..1]; phase 1 forms the
// global means from the slots in rank order and writes the local squared deviations to mine[2..3]; phase 2 (no pass
// over the samples) sums those in rank order and writes out[0].
__global__ __launch_bounds__(PPO_ADV_THREADS) void ppo_explained_variance_kernel(int n, const float* __restrict__ ret, const float* __restrict__ val,
                                                                                int phase, const double* __restrict__ slots, int world,
                                                                                double* __restrict__ mine, double* __restrict__ out) {
  __shared__ double lds[2][PPO_ADV_THREADS];
  const double cnt = (double)(phase < 0 ? 1 : world) * n;
  double sy = 0.0, sd = 0.0, qy = 0.0, qd = 0.0;
  if (phase <= 0) {
    ppo_ev_pass(lds, n, ret, val, false, 0.0, 0.0, &sy, &sd);
    if (phase == 0) {
      if (threadIdx.x == 0) mine[0] = sy, mine[1] = sd;
      return;
    }
  } else {
    for (int r = 0; r < world; ++r) sy += slots[4 * r], sd += slots[4 * r + 1];
  }
  if (phase < 0 || phase == 1) {
    ppo_ev_pass(lds, n, ret, val, true, sy / cnt, sd / cnt, &qy, &qd);
    if (phase == 1) {
      if (threadIdx.x == 0) mine[2] = qy, mine[3] = qd;
      return;
    }
  } else {
    for (int r = 0; r < world; ++r) qy += slots[4 * r + 2], qd += slots[4 * r + 3];
  }
  const double var_y = qy / cnt, var_d = qd / cnt;
  if (threadIdx.x == 0) out[0] = var_y == 0.0 ? (double)__builtin_nanf("") : 1.0 - var_d / var_y;
}

#endif  // __HIPCC__

}  // namespace upkie
