"""The shapes the asymmetric actor-critic (a critic observation of its own) is tested at, and the builders the CPU and GPU
tests share: tests/test_asymmetric_critic.py shows on the host that these inputs tell the feature from its likely bugs,
tests/test_asymmetric_critic_gpu.py runs them on the device, tests/ppo_distributed_worker.py two of the rows under a
process group. Style and helpers of tests/mlp_shapes.py. Below the rows: the layouts, sizes and call lists the privileged
stage is run at."""

from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from tests import asymmetric_reference as AR
from tests import mlp_shapes as S
from upkie_amd.policies import asymmetric_shape, mlp_shape

DEV = S.DEV
T = S.T
BOUNDS = S.DEFAULT_BOUNDS

Row = namedtuple("Row", "N obs_dim actor act_dim critic_obs_dim critic activation why seed", defaults=(0,))

# (N, D, actor widths, A, Dc, critic widths, activation), what the row is there for, and the seed of the default init under
# which the critic's value and first-layer gradient tell the critic's row from the actor's (tests/test_asymmetric_critic.py)
ROWS = [
    Row(17, 3, [16], 2, 5, [16], "tanh", "W16, one tile each, N not a multiple of 16"),
    Row(33, 4, [32], 1, 20, [24, 32], "relu", "critic has two input tiles, actor one; dot head"),
    Row(64, 40, [64, 64], 1, 7, [48], "tanh", "actor input wider than critic's: stale stage rows"),
    Row(100, 4, [16], 1, 129, [64], "relu", "W256 set by Dc alone; nine input tiles; tiny actor in a wide unroll"),
    Row(333, 6, [64, 64], 2, 6, [64, 64], "relu", "Dc = D but different tensors"),
    Row(1001, 5, [40, 24], 3, 12, [40, 24], "tanh", "N and widths off the tile sizes"),
    # the rows below take the symmetric matrix's geometries (tests/mlp_shapes.py) through the critic's own pointer, width,
    # statistics and restage; tests/test_asymmetric_critic.py asserts what they cover
    Row(1, 3, [16], 2, 9, [16], "relu", "W16 relu; N = 1", seed=2),
    Row(1001, 5, [32], 3, 17, [20, 32], "tanh", "W32 tanh; the critic's second input tile holds one word"),
    Row(1000, 16, [128, 128], 2, 24, [128, 128], "relu", "W128 relu; three-wave blocks", seed=1),
    Row(500, 8, [128, 128, 128], 1, 100, [128, 128, 128], "tanh", "W128 tanh; two-wave blocks; the critic's stage is the larger"),
    Row(1000, 30, [256, 256, 128], 36, 48, [256, 256, 128], "tanh",
        "W256 tanh; one-wave blocks above the grid cap: restage, the next chunk's actor stage, partials added to; Dc a multiple of 16"),
    Row(100, 256, [256] * 4, 64, 256, [256] * 4, "relu", "the widest: raised dynamic-LDS limit, one-wave blocks, both inputs 16 full tiles", seed=4),
    Row(333, 255, [64], 6, 7, [64], "tanh", "the actor takes 16 input tiles, the critic one: the most stale rows under the critic's stage"),
    Row(64, 4, [16], 1, 32, [256, 16], "tanh", "Dc = 32 exactly; W256 set by a critic hidden layer alone; three-wave blocks"),
]
DEGENERATE = (4, 5, 8, 10)  # rows run with Dc = D on the same rows and statistics: 8 has three-wave blocks, 10 is above the grid cap


def row_id(row):
    return f"{row.N}-{row.obs_dim}-{row.actor}-{row.act_dim}-{row.critic_obs_dim}-{row.critic}-{row.activation}".replace(" ", "")


def shape_of(row, normalize=False, clip_obs=3.0):
    shape = mlp_shape(S.dims(row.obs_dim, row.actor, row.act_dim), S.dims(row.critic_obs_dim, row.critic, 1), row.activation, normalize, clip_obs)
    return shape if shape.critic_obs_dim else asymmetric_shape(shape)  # (Dc = D: asymmetric all the same)


def row_normalize(index):
    """Half of the rows run with observation normalisation."""
    return index % 2 == 1


def row_modules(row):
    """(actor, critic) of a row on the host, torch's default init under the row's seed."""
    torch.manual_seed(row.seed)
    return S.tower(row.obs_dim, row.actor, row.act_dim, row.activation), S.tower(row.critic_obs_dim, row.critic, 1, row.activation)


def row_statistics(row):
    """((obs_mean, obs_var), (critic_obs_mean, critic_obs_var)) of a normalising policy: two different draws."""
    return S.normalizer_stats(row.obs_dim, row.seed), S.normalizer_stats(row.critic_obs_dim, row.seed + 100)


def _std(var, eps=1e-8):
    return np.sqrt(var.numpy().astype(np.float64) + eps).astype(np.float32).astype(np.float64)  # (fp64 root, stored as fp32)


def row_sources(row, actor, critic, normalize, log_std=-0.5, low=-1.0, high=1.0):
    """The fp64 sources of the row's policy (`MlpActorCritic.sources()` order of an asymmetric policy) from host modules."""
    D, A, Dc = row.obs_dim, row.act_dim, row.critic_obs_dim
    mean, std, cmean, cstd = np.zeros(D), np.ones(D), np.zeros(Dc), np.ones(Dc)
    if normalize:
        (m, var), (cm, cvar) = row_statistics(row)
        mean, std, cmean, cstd = m.numpy().astype(np.float64), _std(var), cm.numpy().astype(np.float64), _std(cvar)
    src = [mean, std, np.full(A, low), np.full(A, high), cmean, cstd, np.broadcast_to(np.asarray(log_std, dtype=np.float64), (A,)).copy()]
    for seq in (actor, critic):
        for m in seq:
            if isinstance(m, nn.Linear):
                src += [m.weight.detach().double().numpy(), m.bias.detach().double().numpy()]
    return src


def policy(row, normalize=False, log_std=None, low=-1.0, high=1.0):
    """(asymmetric MlpActorCritic on the device, actor, critic, log_std) of a row."""
    from upkie_amd.policies import MlpActorCritic

    actor, critic = row_modules(row)
    actor, critic = actor.to(DEV), critic.to(DEV)
    A = row.act_dim
    log_std = torch.full((A,), -0.5, device=DEV) if log_std is None else log_std
    kw = {}
    if normalize:
        (m, var), (cm, cvar) = row_statistics(row)
        kw = dict(obs_mean=m, obs_var=var, critic_obs_mean=cm, critic_obs_var=cvar, clip_obs=3.0)
    pol = MlpActorCritic.from_modules(actor, critic, log_std, torch.full((A,), low), torch.full((A,), high), seed=row.seed, asymmetric=True, **kw)
    return pol, actor, critic, log_std


def row_observations(row, seed=5, scale=1.0, steps=None):
    """(obs, critic_obs): float32, [N, D] and [N, Dc] (or [steps, N, ...]) from the host generator, independent draws."""
    g = torch.Generator().manual_seed(1000 * seed + row.seed)
    lead = (row.N,) if steps is None else (steps, row.N)
    return scale * torch.randn(*lead, row.obs_dim, generator=g), scale * torch.randn(*lead, row.critic_obs_dim, generator=g)


def obs_as_critic_rows(row, obs):
    """The actor's observation where the critic's row belongs, truncated or zero-padded to Dc: what a kernel that handed the
    critic the wrong pointer, width or stage rows would have read."""
    obs = np.asarray(obs, dtype=np.float64)
    out = np.zeros(obs.shape[:-1] + (row.critic_obs_dim,))
    n = min(row.obs_dim, row.critic_obs_dim)
    out[..., :n] = obs[..., :n]
    return out


def row_rollout(row, shape, sources, seed=0, obs_normalized=False):
    """tests/mlp_shapes.py's `row_rollout` with the critic's rows beside the observations (dict of [T, N, ...] float32).
    ``obs_normalized``: the buffer's rows are what the networks read (the update does not normalise them), so the actions,
    log-probs and values are drawn around the networks' outputs on the rows as they are."""
    from upkie_amd import abi

    rng = np.random.default_rng(seed + 10 * row.seed)
    N, A = row.N, row.act_dim
    obs, cobs = (t.numpy() for t in row_observations(row, seed=7, steps=T))
    if obs_normalized:
        shape = abi.UpkieMlpShape.from_buffer_copy(shape)
        shape.normalize = 0
    _, mean, _, value = AR.forward(shape, sources, obs.reshape(T * N, -1).astype(np.float64), cobs.reshape(T * N, -1).astype(np.float64))
    log_std = np.asarray(sources[AR.N_FIXED], dtype=np.float64)
    actions = (mean + np.exp(log_std) * rng.normal(size=(T * N, A))).astype(np.float32)
    from tests import mlp_reference as R

    log_prob = R.log_prob(actions.astype(np.float64), mean, log_std)
    delta = rng.normal(0.0, 0.25, size=T * N)
    for bound in (1.2, 0.8):  # ratio = exp(-delta): keep it >= 1e-3 away from the clip bounds
        near = np.abs(np.exp(-delta) - bound) < 1e-3
        delta[near] += 0.01
    f32 = lambda a, *tail: np.asarray(a, dtype=np.float32).reshape(T, N, *tail)  # noqa: E731
    return {"observations": f32(obs, row.obs_dim), "critic_observations": f32(cobs, row.critic_obs_dim), "actions": f32(actions, A),
            "log_probs": f32(log_prob + delta), "advantages": f32(rng.normal(0.3, 1.0, size=T * N)),
            "returns": f32(value + rng.normal(0.0, 1.0, size=T * N)), "values": f32(value + rng.normal(0.0, 0.2, size=T * N))}


# ---------------------------------------------------------------- the privileged stage's inputs
SEGMENTS = AR.SEGMENTS
PRIVILEGED_MAX_LINKS = 24
_ALL_LINKS = tuple(range(PRIVILEGED_MAX_LINKS))
_BLOCK_EDGES = (1, 63, 64, 65, 129, 1000)  # around the 64 envs of a block: one short of it, exactly it, one more, two blocks and one env

# name, `include`, D, A, the links the model randomises, the batch sizes, the calls after the first reset, the seed of the
# call list. The first is the layout of the Ppo tests; the others are the layouts the kernel serves besides.
Layout = namedtuple("Layout", "name include D A links sizes calls seed", defaults=(0,))
PRIVILEGED_LAYOUTS = [
    Layout("default", SEGMENTS, 4, 2, (1, 2, 5, 12), (1, 65, 1000), 40),
    Layout("reversed", SEGMENTS[::-1], 4, 2, (1, 2, 5, 12), _BLOCK_EDGES, 12),  # the observation last
    Layout("observation-256", ("observation",), 256, 2, (), (1, 65, 1000), 12),  # a 256-word row, no staged column
    Layout("force-alone", ("push_force",), 4, 2, (), (1, 65, 1000), 12),  # no observation segment: a terminal row is the old row
    Layout("27-columns", SEGMENTS, 4, 2, _ALL_LINKS, _BLOCK_EDGES, 12),  # seven passes of the staging loop
    Layout("256-words", ("command", "link_scale", "observation", "push_force"), 200, 29, _ALL_LINKS, (1, 65, 1000), 12),  # 29 + 24 + 200 + 3
]
DEFAULT_LAYOUT = PRIVILEGED_LAYOUTS[0]
NEW_LAYOUTS = PRIVILEGED_LAYOUTS[1:]
PRIVILEGED_SIZES, PRIVILEGED_CALLS = DEFAULT_LAYOUT.sizes, DEFAULT_LAYOUT.calls
PRIVILEGED_D, PRIVILEGED_A, PRIVILEGED_LINKS = DEFAULT_LAYOUT.D, DEFAULT_LAYOUT.A, DEFAULT_LAYOUT.links
# what the calls of a new layout are, in order: a step as Ppo issues it, a step with no final_obs (next_obs stands in), a step
# with no end flags (nothing ended), and resets mid-run under a mixed mask, an all-zero mask and no mask
SCRIPT = ("step", "step", "step_no_final", "reset_mixed", "step", "step_no_flags", "reset_zero", "step", "reset_all", "step", "step_no_final", "step")


def layout_dim(layout):
    counts = {"observation": layout.D, "command": layout.A, "push_force": 3, "link_scale": len(layout.links)}
    return sum(counts[k] for k in layout.include)


def layout_cases(layouts=None):
    """[(layout, num_envs)] of the layouts (default: the new ones) at their sizes, and the ids."""
    cases = [(lay, n) for lay in (NEW_LAYOUTS if layouts is None else layouts) for n in lay.sizes]
    return cases, [f"{lay.name}-{n}" for lay, n in cases]


def end_rate(num_envs):
    """Ends per env and step of a new layout's call list: enough for every size above 1 to see both kinds of end."""
    return min(0.5, max(0.08, 4.0 / num_envs))


def privileged_calls(num_envs, seed=0, calls=PRIVILEGED_CALLS, layout=DEFAULT_LAYOUT, rate=0.05, script=None):
    """The inputs of `calls` calls of the privileged stage after a reset (element 0): per call next_obs and a final_obs that
    differs from it [N, D], the command [N, A], the force [3, N] and link scales [24, N] as the events would have left them
    (rewritten between calls; zero force and fresh scales where the episode ended) and end flags at about `rate` per step.
    With a ``script`` (one of `SCRIPT`'s words per call) a call also carries its "op" and, for a reset, its "mask"; only
    a step that passes end flags ends an episode."""
    rng = np.random.default_rng(100 * seed + num_envs)
    N, D, A = num_envs, layout.D, layout.A
    f = lambda *shape: rng.normal(size=shape).astype(np.float32)  # noqa: E731
    scale = (1.0 + 0.2 * rng.uniform(-1, 1, size=(PRIVILEGED_MAX_LINKS, N))).astype(np.float32)
    out = []
    for k in range(calls + 1):
        op = script[k - 1] if script is not None and k else "step"
        ended = rng.uniform(size=N) < (rate if k and op in ("step", "step_no_final") else 0.0)
        terminated = ended & (rng.uniform(size=N) < 0.5)
        truncated = ended & ~terminated
        force = (f(3, N) * (rng.uniform(size=N) < 0.5)).astype(np.float32)
        force[:, ended] = 0.0
        scale = scale.copy()
        scale[:, ended] = (1.0 + 0.2 * rng.uniform(-1, 1, size=(PRIVILEGED_MAX_LINKS, int(ended.sum())))).astype(np.float32)
        out.append({"next_obs": f(N, D), "final_obs": f(N, D), "command": f(N, A), "force": force, "link_scale": scale,
                    "terminated": terminated.astype(np.uint8), "truncated": truncated.astype(np.uint8)})
        if script is not None:
            mixed = (rng.uniform(size=N) < 0.5).astype(np.uint8)
            out[-1].update(op=op, mask={"reset_mixed": mixed, "reset_zero": np.zeros(N, dtype=np.uint8)}.get(op))
    return out


def layout_calls(layout, num_envs):
    """The call list of a (layout, size) of `PRIVILEGED_LAYOUTS`: the default's 40 plain steps, or `SCRIPT`."""
    if layout is DEFAULT_LAYOUT:
        return privileged_calls(num_envs)
    assert layout.calls == len(SCRIPT)
    return privileged_calls(num_envs, seed=layout.seed, calls=layout.calls, layout=layout, rate=end_rate(num_envs), script=SCRIPT)


def run_privileged_twin(num_envs, calls, mutation=None, layout=DEFAULT_LAYOUT):
    """(observation, final_observation) after each call of `privileged_calls`' list on the twin."""
    twin = AR.PrivilegedTwin(num_envs, layout.D, layout.A, layout.links, include=layout.include, mutation=mutation)
    first = calls[0]
    twin.reset(first["next_obs"], first["command"], first["force"], first["link_scale"])
    rows = [(twin.observation.copy(), None)]
    for c in calls[1:]:
        op = c.get("op", "step")
        if op.startswith("reset"):
            twin.reset(c["next_obs"], c["command"], c["force"], c["link_scale"], mask=c["mask"])
        else:
            flags = (None, None) if op == "step_no_flags" else (c["terminated"], c["truncated"])
            twin.step(c["next_obs"], None if op == "step_no_final" else c["final_obs"], c["command"], c["force"], c["link_scale"], *flags)
        rows.append((twin.observation.copy(), twin.final_observation.copy()))
    return rows
