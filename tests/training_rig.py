"""The rig of the driver tests on the GPU (`Ppo`, `Distillation`, the evaluator around them): the pendulum env, the small
towers, the stand-in reward, the warm-up step a graphed driver takes before it captures, a snapshot of everything a run
leaves behind and its bit-for-bit comparison. A plain module: every test file passes its own sizes, seeds and widths."""

import numpy as np
import torch
import torch.nn as nn


def pendulum(num_envs, limit, seed=None, pitch=0.3, model=None):
    """The vectorised pendulum env with the same-step autoreset and episodes of at most ``limit`` steps (``seed`` and
    ``model``: given to the env only when set)."""
    import upkie_amd.envs as envs
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    init = RobotState(randomization=RobotStateRandomization(pitch=pitch))
    kw = {k: v for k, v in (("seed", seed), ("model", model)) if v is not None}
    return envs.make("Upkie-HIP-Pendulum-Vec", num_envs=num_envs, frequency=200.0, init_state=init, autoreset_mode="same_step",
                     max_episode_steps=limit, **kw)


def reset_pendulum(num_envs, seed=0, limit=400, pitch=0.1):
    """`pendulum` after ``reset(seed=seed)``: the env of the loops that step it by hand."""
    env = pendulum(num_envs, limit, pitch=pitch)
    env.reset(seed=seed)
    return env


def tower(d_in, d_out, width=16, hidden=2):
    """A tanh tower of ``hidden`` layers of ``width`` units (built in order: the same ``torch.manual_seed``, the same weights)."""
    sizes = [d_in] + [width] * hidden
    layers = [m for a, b in zip(sizes[:-1], sizes[1:]) for m in (nn.Linear(a, b), nn.Tanh())]
    return nn.Sequential(*layers, nn.Linear(width, d_out))


def pitch_reward(obs, info):
    """The examples' stand-in reward: 1 - |pitch|."""
    return torch.abs(obs[:, 0]).neg_().add_(1.0)


def warm_up_as_the_capture_does(model):
    """A graphed driver runs one real rollout step into the last slot before it captures; the same by hand."""
    model._setup()
    model._slot = model.n_steps - 1
    model._rollout_step()


def snapshot(model, extra=()):
    """``(state, records)``: clones of the driver's state tensors, of every normaliser it has and of the members ``extra``
    names (``"buffer.rewards"``, ``"labels"``, ...), and copies of its records."""
    torch.cuda.synchronize()
    state = {k: v.clone() for k, v in model._state_tensors().items()}
    for name in ("normalizer", "critic_normalizer"):
        norm = getattr(model, name, None)
        if norm is not None:
            state[name] = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in norm.state_dict().items()}
    for name in extra:
        member = model
        for part in name.split("."):
            member = getattr(member, part)
        state[name] = member.clone()
    return state, [dict(r) for r in model.records]


def same(a, b):
    """Equal bit for bit (tensors), key by key and item by item (dicts, lists), NaN equal to NaN (numbers)."""
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b or (a != a and b != b)


def np64(t):
    return t.detach().double().cpu().numpy()


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- a stage alone, on a handle that is never stepped
def events_stage(model, num_envs, offset, seed, **settings):
    """A simulation handle that is never stepped, and the `EpisodeEvents` stage on it."""
    import types

    from upkie_amd import abi
    from upkie_amd.events import EpisodeEvents
    from upkie_amd.sim import BatchedSim

    cfg = abi.default_sim_config(num_envs, seed=seed)
    cfg.env_id_offset = offset
    sim = BatchedSim(cfg, model.struct)
    env = types.SimpleNamespace(sim=sim, model=model, num_envs=num_envs, device=sim.device)
    return sim, EpisodeEvents(env, **settings)


def read_state(stage):
    """A stage's `state_tensors` on the host."""
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in stage.state_tensors().items()}


def check_event_records(got, want, envs):
    np.testing.assert_allclose(got["link_scale"][:, envs], want["link_scale"][:, envs], atol=1e-6, rtol=0.0)
    np.testing.assert_allclose(got["body_inertials"][:, envs].astype(np.float64), want["body_inertials"][:, envs], rtol=3e-5, atol=1e-9)
