"""The shapes the MLP kernels (policy launch, time-limit bootstrap, PPO gradient launch A) are tested at, and the builders
the tests share: plain data plus torch modules with the default init.

`CASES` and `WIDEST` are the symmetric shapes of tests/test_mlp_policy_gpu.py, tests/test_time_limits_gpu.py and
tests/test_ppo_gpu.py. `MATRIX` holds them again as rows with a critic of their own, plus the rows that reach the
instantiations, block geometries and edges those leave out; tests/test_mlp_shape_matrix.py asserts that the table covers
what it claims, tests/test_mlp_shape_matrix_gpu.py runs every row on the device."""

from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from tests import mlp_reference as R
from upkie_amd.policies import MlpActorCritic, mlp_shape

DEV = "cuda:0"
T = 2  # rollout steps of the gradient tests: the buffers are [T, N, ...]

# (N, obs_dim, hidden widths (both towers), act_dim, activation)
CASES = [
    (4096, 4, [64, 64], 1, "tanh"),
    (333, 6, [64, 64], 2, "relu"),
    (1000, 30, [256, 256, 128], 36, "tanh"),
    (1, 3, [16], 2, "relu"),
    (1001, 5, [40, 24], 3, "tanh"),  # N not a multiple of 16 or 32, widths not of 16
]
IDS = [f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}" for c in CASES]
# the widest shape upkie_mlp_packed_words accepts: one tile's LDS stage (88 KiB) is above the 64 KiB default, so the
# gradient launch runs one-wave blocks with the raised dynamic-LDS limit
WIDEST = (100, 256, [256, 256, 256, 256], 64, "relu")

# The project's bounds of the quantities the matrix checks (tests/test_mlp_policy_gpu.py, tests/test_ppo_gpu.py): absolute
# on mean and value, relative Frobenius per gradient tensor. A row may carry bounds of its own in `bounds` (same keys),
# each at most four times torch fp32's distance to the fp64 twin on that row (profiles/mlp_shape_matrix.txt), with the
# reason beside it.
DEFAULT_BOUNDS = {"mean": 1e-5, "value": 1e-5, "norm_obs": 1e-6, "log_prob": 1e-4, "grad": 1e-5}

Row = namedtuple("Row", "N obs_dim actor act_dim critic activation why seed bounds", defaults=("", 0, None))


def _symmetric(case, why, seed=0):
    N, D, widths, A, act = case
    return Row(N, D, list(widths), A, list(widths), act, why, seed)


# (N, obs_dim, actor widths, act_dim, critic widths, activation), then what the row is there for
# and, where the default init under seed 0 leaves a last unit dead (ReLU) or nearly unused, the seed that does not
# (tests/test_mlp_shape_matrix.py demands every layer's last units to be seen)
MATRIX = [_symmetric(c, "the symmetric cases of the policy, bootstrap and gradient tests", seed=2 if c[0] == 1 else 0) for c in CASES] + [
    _symmetric(WIDEST, "the widest shape: one-wave blocks, raised dynamic-LDS limit, sixteen input tiles", seed=4),
    Row(17, 3, [16], 2, [16], "tanh", "W16 tanh"),
    Row(333, 16, [16, 16, 16, 16], 16, [16], "relu", "W16; four layers; every tile exactly full; 16-wide MFMA head"),
    Row(1001, 5, [32], 3, [20, 32], "tanh", "W32 tanh; PAIR = 2 with one real tile"),
    Row(15, 17, [24, 17], 1, [32], "relu", "W32 relu; two first-layer tiles, the second has one word; dot head"),
    Row(256, 40, [64, 64], 1, [48], "tanh", "the pipeline example's 40-word stack; asymmetric towers", seed=1),
    Row(1000, 16, [128, 128], 2, [128, 128], "relu", "W128 relu; nw = 3", seed=1),
    Row(500, 8, [128, 128, 128], 1, [128, 128, 128], "tanh", "W128 tanh; nw = 2"),
    Row(100, 129, [100], 17, [128, 72], "relu", "W256 set by obs_dim; 9 input tiles (second load chunk, clamped loads); 17 actions"),
    Row(333, 255, [64], 6, [64], "tanh", "the 255-word stack of the agent pipeline"),
    Row(64, 4, [16], 1, [256, 16], "tanh", "W256 set by the critic alone; a tiny actor inside a wide unroll"),
    Row(33, 6, [32], 64, [32], "relu", "W64 set by act_dim alone; four action tiles"),
]


def bounds(row):
    return dict(DEFAULT_BOUNDS, **(row.bounds or {}))


def dims(d_in, widths, d_out):
    """[(out, in)] per layer of a tower, head last: `mlp_shape`'s argument."""
    return [(w, n) for w, n in zip(list(widths) + [d_out], [d_in] + list(widths))]


def shape_of(row, normalize=False, clip_obs=3.0):
    return mlp_shape(dims(row.obs_dim, row.actor, row.act_dim), dims(row.obs_dim, row.critic, 1), row.activation, normalize, clip_obs)


def width_class(shape):
    """The template argument W of the shape, as the layout twin (tests/mlp_reference.py) has it; its packed size is held
    to `upkie_mlp_packed_words` on every row by tests/test_mlp_shape_matrix.py."""
    return R._layout(shape)["W"]


def row_id(row):
    return f"{row.N}-{row.obs_dim}-{row.actor}-{row.act_dim}-{row.critic}-{row.activation}".replace(" ", "")


def tower(d_in, widths, d_out, act):
    mods, n = [], d_in
    for w in widths:
        mods += [nn.Linear(n, w), nn.Tanh() if act == "tanh" else nn.ReLU()]
        n = w
    return nn.Sequential(*mods, nn.Linear(n, d_out))


def normalizer_stats(D, seed):
    """(obs_mean, obs_var) of a normalising policy."""
    g = torch.Generator().manual_seed(seed + 1)
    return 0.3 * torch.randn(D, generator=g), torch.rand(D, generator=g) * 3 + 0.2


def policy(D, widths, A, act, seed=0, normalize=False, log_std=None, low=-1.0, high=1.0, critic_widths=None):
    """(MlpActorCritic on the device, actor, critic, log_std): the towers with torch's default init under `seed`."""
    torch.manual_seed(seed)
    actor = tower(D, widths, A, act).to(DEV)
    critic = tower(D, widths if critic_widths is None else critic_widths, 1, act).to(DEV)
    log_std = torch.full((A,), -0.5, device=DEV) if log_std is None else log_std
    kw = {}
    if normalize:
        mean, var = normalizer_stats(D, seed)
        kw = dict(obs_mean=mean, obs_var=var, clip_obs=3.0)
    pol = MlpActorCritic.from_modules(actor, critic, log_std, torch.full((A,), low), torch.full((A,), high), seed=seed, **kw)
    return pol, actor, critic, log_std


def sources_of(pol):
    return [t.detach().double().cpu().numpy() for t in pol.sources()]


# ---------------------------------------------------------------- the matrix's rows without a device
def row_modules(row):
    """(actor, critic) of a row on the host: the modules `policy(..., seed=row.seed)` moves to the device."""
    torch.manual_seed(row.seed)
    return tower(row.obs_dim, row.actor, row.act_dim, row.activation), tower(row.obs_dim, row.critic, 1, row.activation)


def row_normalize(index):
    """Half of the rows run with observation normalisation."""
    return index % 2 == 1


def row_sources(row, actor, critic, normalize, log_std=-0.5, low=-1.0, high=1.0, eps=1e-8):
    """The fp64 sources of the row's policy (`MlpActorCritic.sources()` order) from host modules."""
    D, A = row.obs_dim, row.act_dim
    mean, std = np.zeros(D), np.ones(D)
    if normalize:
        m, var = normalizer_stats(D, row.seed)
        mean = m.numpy().astype(np.float64)
        std = np.sqrt(var.numpy().astype(np.float64) + eps).astype(np.float32).astype(np.float64)  # (fp64 root, stored as fp32)
    src = [mean, std, np.full(A, low), np.full(A, high), np.full(A, log_std)]
    for seq in (actor, critic):
        for m in seq:
            if isinstance(m, nn.Linear):
                src += [m.weight.detach().double().numpy(), m.bias.detach().double().numpy()]
    return src


def row_observations(row, seed=5, scale=1.0, steps=None):
    """float32 observations of a row, [N, D] or [steps, N, D], from the host generator (the same on every machine)."""
    g = torch.Generator().manual_seed(1000 * seed + row.seed)
    size = (row.N, row.obs_dim) if steps is None else (steps, row.N, row.obs_dim)
    return scale * torch.randn(*size, generator=g)


def row_rollout(row, shape, sources, seed=0):
    """A full rollout of T x N samples for the gradient tests, float32 on the host: observations, actions drawn around
    the twin's mean, old values and log-probs perturbed so that ratios clip on both sides but none lies within 1e-3 of a
    clip bound, advantages and returns. (dict of arrays shaped [T, N, ...])"""
    rng = np.random.default_rng(seed + 10 * row.seed)
    N, A = row.N, row.act_dim
    obs = row_observations(row, seed=7, steps=T).numpy()
    _, mean, value = R.forward(shape, sources, obs.reshape(T * N, -1).astype(np.float64))
    log_std = np.asarray(sources[4], dtype=np.float64)
    actions = (mean + np.exp(log_std) * rng.normal(size=(T * N, A))).astype(np.float32)
    log_prob = R.log_prob(actions.astype(np.float64), mean, log_std)
    delta = rng.normal(0.0, 0.25, size=T * N)
    for bound in (1.2, 0.8):  # ratio = exp(-delta): keep it >= 1e-3 away from the clip bounds
        near = np.abs(np.exp(-delta) - bound) < 1e-3
        delta[near] += 0.01
    f32 = lambda a, *tail: np.asarray(a, dtype=np.float32).reshape(T, N, *tail)  # noqa: E731
    return {"observations": f32(obs, row.obs_dim), "actions": f32(actions, A), "log_probs": f32(log_prob + delta),
            "advantages": f32(rng.normal(0.3, 1.0, size=T * N)), "returns": f32(value + rng.normal(0.0, 1.0, size=T * N)),
            "values": f32(value + rng.normal(0.0, 0.2, size=T * N))}


# ---------------------------------------------------------------- a trainer's case: policy, full buffer, state
def trainer_case(case, seed=0, first=False, normalize=False):
    """Policy (built from modules), a full rollout buffer of T x N samples whose actions, values and log-probs come from
    the policy, perturbed old log-probs (none within 1e-3 of a clip bound unless `first`: every ratio is then 1)."""
    from upkie_amd.rollout import RolloutBuffer

    N, D, widths, A, act = case
    torch.manual_seed(seed)
    actor, critic = tower(D, widths, A, act).to(DEV), tower(D, widths, 1, act).to(DEV)
    log_std = nn.Parameter(torch.full((A,), -0.5, device=DEV))
    kw = {}
    if normalize:
        g = torch.Generator().manual_seed(seed + 1)
        kw = dict(obs_mean=0.3 * torch.randn(D, generator=g), obs_var=torch.rand(D, generator=g) * 3 + 0.2, clip_obs=3.0)
    pol = MlpActorCritic.from_modules(actor, critic, log_std, torch.full((A,), -1.0), torch.full((A,), 1.0), seed=seed, **kw)
    buf = RolloutBuffer(T, N, obs_shape=(D,), action_shape=(A,), device=DEV)
    gen = torch.Generator(DEV).manual_seed(seed + 7)
    buf.observations.copy_(torch.randn(T, N, D, device=DEV, generator=gen))
    for t in range(T):
        pol.act(buf.observations[t], out={"action": buf.actions[t], "value": buf.values[t], "log_prob": buf.log_probs[t]})
    rng = np.random.default_rng(seed)
    if not first:
        delta = rng.normal(0.0, 0.25, size=(T, N))
        for bound in (1.2, 0.8):  # ratio = exp(-delta): keep it >= 1e-3 away from the clip bounds
            near = np.abs(np.exp(-delta) - bound) < 1e-3
            delta[near] += 0.01
        buf.log_probs.add_(torch.as_tensor(delta, dtype=torch.float32, device=DEV))
    buf.advantages = torch.as_tensor(rng.normal(0.3, 1.0, size=(T, N)), dtype=torch.float32, device=DEV)
    buf.returns = (buf.values + torch.as_tensor(rng.normal(0.0, 1.0, size=(T, N)), dtype=torch.float32, device=DEV)).contiguous()
    buf.values.add_(torch.as_tensor(rng.normal(0.0, 0.2, size=(T, N)), dtype=torch.float32, device=DEV))
    buf.pos, buf.full = T, True
    return pol, actor, critic, log_std, buf


def trainer_state(pol, tr):
    return [pol.packed.clone(), tr.m.clone(), tr.v.clone(), tr.scalars.clone()]


def restore_trainer(pol, tr, st):
    for dst, src in zip((pol.packed, tr.m, tr.v, tr.scalars), st):
        dst.copy_(src)
