"""fp64 twins of the distillation update and of the DAgger mix (csrc/distill.hpp, csrc/distill_mix.hpp; include/upkie_hip.h,
"Policy distillation"), and the inputs tests/test_distill_gpu.py drives the kernels with.

* `minibatch` -- the behaviour-cloning loss ``mean((mu - label)^2)`` of the unclamped Gaussian mean and its gradient by the
  hand-written backpropagation of tests/ppo_reference.py (`_forward` / `_backward`); `update` -- whole epochs of
  minibatches with ``clip_grad_norm_`` and Adam (`ppo_reference.adam_step`). Gradients and parameters are lists over the
  trainable sources as there: log_std, then (weight, bias) per layer of the actor and of the critic; everything but the
  actor's entries is zero (the gradient) or unchanged (the parameters).
* `MixTwin` -- the mix, numpy, with the Philox of tests/episode_events_reference.py.
* ``mutation=``: a one-line mistake the GPU tests' inputs have to tell from the feature (tests/test_distill.py)."""

import math

import numpy as np

from tests import episode_events_reference as ER
from tests import mlp_shapes as S
from tests import ppo_reference as PR

STREAM_DISTILL = 8
MUTATIONS = ("no_one_over_a", "clamped_mean", "label_unpermuted", "critic_gradient")
MIX_MUTATIONS = ("drove_inverted",)
LABEL_NOISE = 0.5  # std of the noise on the GPU tests' labels
ACTION_BOUND = 0.01  # the GPU tests' students clamp at +-0.01: the means exceed it, so a clamped mean shows
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-5)


def split(shape, sources):
    """(mean, std, low, high, log_std, actor [(W, b)], critic [(W, b)]) in fp64 from `MlpActorCritic.sources()`, symmetric
    (4 fixed tensors) or asymmetric (6: the critic's statistics after the action bounds; its first layer reads Dc words)."""
    src = [np.asarray(s, dtype=np.float64).reshape(-1) for s in sources]
    Dc = int(shape.critic_obs_dim)
    nf = 6 if Dc else 4
    mean, std, low, high, log_std = src[0], src[1], src[2], src[3], src[nf]
    rest = src[nf + 1:]

    def tower(rest, n_in, layers, widths, outputs):
        out = []
        for w in list(widths[:layers]) + [outputs]:
            out.append((rest[0].reshape(int(w), n_in), rest[1]))
            rest, n_in = rest[2:], int(w)
        return out, rest

    actor, rest = tower(rest, int(shape.obs_dim), int(shape.actor_layers), shape.actor_widths, int(shape.act_dim))
    critic, rest = tower(rest, Dc or int(shape.obs_dim), int(shape.critic_layers), shape.critic_widths, 1)
    assert not rest
    return mean, std, low, high, log_std, actor, critic


def trainable(shape, sources):
    _, _, _, _, log_std, actor, critic = split(shape, sources)
    out = [log_std]
    for W, b in actor + critic:
        out += [W, b]
    return out


def actor_slice(shape):
    """Where the actor's tensors sit in a `trainable` list."""
    return slice(1, 1 + 2 * (int(shape.actor_layers) + 1))


def normalized(shape, sources, obs, obs_normalized=False):
    mean, std = split(shape, sources)[:2]
    x = np.asarray(obs, dtype=np.float64).reshape(len(obs), -1)
    if shape.normalize and not obs_normalized:
        x = np.clip((x - mean) / std, -float(shape.clip_obs), float(shape.clip_obs))
    return x


def mean_of(shape, sources, obs, obs_normalized=False):
    """The actor's unclamped mean [B, A], fp64."""
    actor = split(shape, sources)[5]
    return PR._forward(shape, actor, normalized(shape, sources, obs, obs_normalized))[-1]


def minibatch(shape, sources, obs, labels, obs_normalized=False, mutation=None):
    """(loss, gradient list, its norm) of one minibatch: ``obs`` [B, D] and ``labels`` [B, A] already gathered."""
    _, _, low, high, log_std, actor, critic = split(shape, sources)
    x = normalized(shape, sources, obs, obs_normalized)
    y = np.asarray(labels, dtype=np.float64).reshape(len(x), -1)
    B, A = y.shape
    hs = PR._forward(shape, actor, x)
    mu = np.clip(hs[-1], low, high) if mutation == "clamped_mean" else hs[-1]
    e = mu - y
    loss = float(np.mean(e * e))
    dz = 2.0 * e / (B if mutation == "no_one_over_a" else B * A)
    grads = [np.zeros_like(log_std)]
    for W_b in PR._backward(shape, actor, hs, dz):
        grads += list(W_b)
    if mutation == "critic_gradient":  # (the critic's tower run on the same rows under a loss of its own)
        hc = PR._forward(shape, critic, x if not int(shape.critic_obs_dim) else np.ones((B, int(shape.critic_obs_dim))))
        for W_b in PR._backward(shape, critic, hc, 2.0 * hc[-1] / B):
            grads += list(W_b)
    else:
        for W, b in critic:
            grads += [np.zeros_like(W), np.zeros_like(b)]
    norm = math.sqrt(sum(float(np.sum(g * g)) for g in grads))
    return loss, grads, norm


def gather(obs, labels, perm, start, size, mutation=None):
    """Minibatch [start, start + size) of a permutation over the flattened rows."""
    idx = np.asarray(perm[start:start + size], dtype=np.int64)
    rows = np.arange(start, start + size) if mutation == "label_unpermuted" else idx
    return np.asarray(obs, dtype=np.float64)[idx], np.asarray(labels, dtype=np.float64)[rows]


def update(shape, sources, obs, labels, perms, batch_size, lr=1e-3, max_grad_norm=1.0, state=None, obs_normalized=False, mutation=None, trace=None):
    """``len(perms)`` epochs of minibatches of ``batch_size`` over ``obs`` [total, D], ``labels`` [total, A]. Returns
    (sources after, state (m, v, t), stats [epochs, minibatches, 3] of (loss, norm, clip coefficient), the gradients of
    the first minibatch). ``state``: (m, v, t) to continue from (None: a fresh optimiser). ``trace``: a list that gets
    (parameters before the step, gradients, clip coefficient) of every minibatch, in order."""
    sources = [np.array(s, dtype=np.float64) for s in sources]
    nf = 6 if int(shape.critic_obs_dim) else 4
    params = trainable(shape, sources)
    m, v, t = state if state is not None else ([0 * p for p in params], [0 * p for p in params], 0)
    total = len(obs)
    stats, first = [], None
    for perm in perms:
        row = []
        for start in range(0, total, batch_size):
            x, y = gather(obs, labels, perm, start, min(batch_size, total - start), mutation)
            loss, grads, norm = minibatch(shape, sources, x, y, obs_normalized, mutation)
            first = grads if first is None else first
            if trace is not None:
                trace.append((params, grads, min(1.0, max_grad_norm / (norm + 1e-6))))
            params, m, v, t = PR.adam_step(params, grads, m, v, t, max_grad_norm, lr, **ADAM)
            for k, p in enumerate(params):
                sources[nf + k] = p.reshape(np.shape(sources[nf + k]))
            row.append([loss, norm, min(1.0, max_grad_norm / (norm + 1e-6))])
        stats.append(row)
    return sources, (m, v, t), np.array(stats), first


def step_bound(p0, g, coef, lr, grad_bound=1e-5):
    """tests/test_ppo_gpu.py's bound on one Adam step from a fresh state (test_one_full_update_against_the_fp64_twin),
    word by word: a gradient error delta (relative ``grad_bound`` of the tensor's norm, plus 1e-6 of the word) moves the
    step by about lr delta / (|g| + eps); then the rounding of the word itself."""
    delta = grad_bound * np.linalg.norm(g) * coef + 1e-6 * np.abs(g) * coef
    return lr * delta / (np.abs(g) * coef + 1e-5) + 2e-7 * np.abs(p0) + 1e-9


# ---------------------------------------------------------------- the GPU tests' inputs
def teacher_sources(row, normalize):
    """The fp64 sources of a policy of the row's architecture built from ANOTHER seed: what the labels come from."""
    import torch

    torch.manual_seed(row.seed + 100)
    actor, critic = S.tower(row.obs_dim, row.actor, row.act_dim, row.activation), S.tower(row.obs_dim, row.critic, 1, row.activation)
    return S.row_sources(row, actor, critic, normalize)


def gpu_labels(row, shape, observations, normalize, seed=0):
    """float32 labels [T N, A] of the gradient tests: the twin's mean of the other-seed policy on the same rows, plus
    N(0, LABEL_NOISE) noise."""
    rng = np.random.default_rng(77 + seed + 10 * row.seed)
    mean = mean_of(shape, teacher_sources(row, normalize), observations)
    return (mean + rng.normal(0.0, LABEL_NOISE, size=mean.shape)).astype(np.float32)


# ---------------------------------------------------------------- the mix
MIX_SIZES = (1, 63, 64, 65, 257)
MIX_ACTIONS = (1, 3, 16, 17, 64)
MIX_BETAS = (0.0, 0.5, 1.0)
MIX_CALLS = 40
MIX_SEED = 0x1234_5678_9ABC
MIX_OFFSET = (1 << 32) - 40  # ids that cross 2^32 inside every batch of more than 40 envs


def mix_inputs(num_envs, act_dim, call, offset=0):
    """(label, student_action) [N, A] float32 of call ``call``, a function of the GLOBAL env id (so that shards see the
    rows of their envs), both reaching past the bounds on both sides; (low, high) [A]."""
    ids = (np.arange(num_envs, dtype=np.uint64) + np.uint64(offset)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    a = np.arange(act_dim, dtype=np.float64)
    phase = (ids % np.uint64(1000)).astype(np.float64)[:, None]
    label = np.sin(0.37 * phase + 0.61 * a + 0.05 * call) * 1.5
    student = np.cos(0.23 * phase + 0.41 * a + 0.07 * call) * 1.5
    return label.astype(np.float32), student.astype(np.float32)


def mix_bounds(act_dim):
    a = np.arange(act_dim, dtype=np.float64)
    return (-1.0 + 0.01 * a).astype(np.float32), (0.5 + 0.02 * a).astype(np.float32)


def threshold(beta):
    return int(math.floor(float(beta) * 16777216.0 + 0.5))


class MixTwin:
    """The mix for ``num_envs`` envs with global ids ``env_id_offset + n`` under the sim's ``seed``."""

    def __init__(self, num_envs, low, high, seed=0, env_id_offset=0, beta=0.0, mutation=None):
        self.num_envs, self.seed, self.mutation = int(num_envs), int(seed), mutation
        ids = np.arange(num_envs, dtype=np.uint64) + np.uint64(env_id_offset)
        self.lo, self.hi = (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32), (ids >> np.uint64(32)).astype(np.uint32)
        self.low, self.high = np.asarray(low, dtype=np.float32), np.asarray(high, dtype=np.float32)
        self.calls = np.zeros(num_envs, dtype=np.uint32)
        self.threshold = threshold(beta)

    def step(self, label, student_action):
        """(applied [N, A] float32, drove [N] uint8)."""
        r = ER.philox4x32_10(self.lo, self.hi, self.calls, np.uint32(STREAM_DISTILL << 24), self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF)
        self.calls = self.calls + np.uint32(1)
        teacher = (r[0] >> np.uint32(8)).astype(np.int64) < self.threshold
        if self.mutation == "drove_inverted":
            teacher = ~teacher
        rows = np.where(teacher[:, None], np.asarray(label, dtype=np.float32), np.asarray(student_action, dtype=np.float32))
        return np.minimum(np.maximum(rows, self.low), self.high).astype(np.float32), teacher.astype(np.uint8)


def gradient_case(index, row):
    """What the gradient test runs row ``index`` of tests/mlp_shapes.py's MATRIX on: (shape, the student's fp64 sources,
    observations [T N, D] float32 (`row_rollout`'s), labels [T N, A] float32); half of the rows normalise."""
    normalize = S.row_normalize(index)
    shape = S.shape_of(row, normalize=normalize)
    sources = S.row_sources(row, *S.row_modules(row), normalize, low=-ACTION_BOUND, high=ACTION_BOUND)
    obs = S.row_rollout(row, shape, sources)["observations"].reshape(S.T * row.N, row.obs_dim)
    return shape, sources, obs, gpu_labels(row, shape, obs, normalize)


def mix_cases():
    """(num_envs, act_dim) of the mix test, every size with every width; ids start at MIX_OFFSET."""
    return [(n, a) for n in MIX_SIZES for a in MIX_ACTIONS]


def actor_plan(shape):
    """tests/ppo_reference.py's `plan` with the trainable span distill_plan (csrc/distill.hpp) gives the launch: the
    actor's words, from its first weight word to the critic's first, and the grid cap and fold blocks that follow."""
    lay = PR.R._layout(shape)
    p = dict(PR.plan(shape))
    p["train_off"] = lay["actor"][0][1]
    p["train_words"] = lay["critic"][0][1] - p["train_off"]
    p["grid_cap"] = min(PR.MAX_GRID, max(1, PR.PARTIAL_CAP_BYTES // (4 * p["train_words"])))
    p["fold_blocks"] = (p["train_words"] + PR.FOLD_THREADS - 1) // PR.FOLD_THREADS
    return p
