"""Recording doubles for the stages around an agent step (the policy, the pipeline, the normaliser, the episode
statistics, the reward, the evaluation tally) and a recorder around the CPU oracle env: what tests/test_ppo_rollout_step.py
and tests/test_agent_step.py drive `Ppo` and `PolicyEvaluator` with. Every double logs its calls, in order and with the
argument OBJECTS, in one `Calls`. And host stand-ins for the stages a driver saves (`stage`, `saved_parts`): what the
file-layout tests of `Ppo` (tests/test_ppo_learn.py) and `Distillation` (tests/test_distill.py) save and load."""

import types

import torch

N, T, K, D, A = 3, 5, 2, 4, 1  # envs, steps, stacked frames, raw observation words, action words


class Calls:
    """The log of the doubles: the names in call order, and per name the arguments of every call."""

    def __init__(self):
        self.names, self.args = [], {}

    def add(self, name, **args):
        self.names.append(name)
        self.args.setdefault(name, []).append(args)


class Env:
    """The oracle env behind a recorder of what `step` is given and what it returns (and of `reset`)."""

    def __init__(self, env, calls):
        self._env, self.calls, self.num_envs = env, calls, env.num_envs

    def __getattr__(self, name):  # (`device`, `autoreset_mode`, `observation`, ...: the oracle env's)
        return getattr(self._env, name)

    def reset(self, **kw):
        out = self._env.reset(**kw)
        self.calls.add("env.reset", out=out, **kw)
        return out

    def step(self, action):
        out = self._env.step(action)
        self.calls.add("env.step", action=action, out=out, ended=out[2].clone() | out[3].clone(), truncated=out[3].clone(), reward=out[1].clone())
        return out


class Policy:
    def __init__(self, obs_dim, calls):
        self.shape, self.calls = types.SimpleNamespace(obs_dim=obs_dim, act_dim=A), calls

    def act(self, obs, out):
        self.calls.add("act", obs=obs, out=out, seen=obs.clone())
        out["env_action"].fill_(0.5)
        if "action" in out:
            out["action"].fill_(0.5)
        return out["env_action"], out.get("action"), out.get("value"), out.get("log_prob")

    def mean_action(self, obs, out):
        self.calls.add("mean_action", obs=obs, out=out)
        out.fill_(0.25)

    def bootstrap_time_limits(self, final_obs, terminated, truncated, reward, gamma):
        self.calls.add("bootstrap", final_obs=final_obs, terminated=terminated, truncated=truncated, reward=reward, gamma=gamma)

    def value(self, obs):
        self.calls.add("value", obs=obs)
        return torch.zeros(N)


class _NoiseCounters:
    def __init__(self, log):
        self.log = log

    def zero_(self):
        self.log.add("pipeline.calls.zero_")


class Pipeline:
    def __init__(self, calls):
        self.num_envs, self.obs_dim, self.act_dim, self.stack = N, D, A, K
        self.frame_dim, self.stacked_dim = D + A, K * (D + A)
        self.observation, self.final_observation, self.command = torch.zeros(N, self.stacked_dim), torch.zeros(N, self.stacked_dim), torch.zeros(N, A)
        self.log, self.calls = calls, _NoiseCounters(calls)  # (`calls` is what an `AgentPipeline` names its noise counters)

    def reset(self, obs):
        self.log.add("pipeline.reset", obs=obs)
        self.observation[:, :D] = obs
        return self.observation

    def shape_action(self, env_action):
        self.log.add("shape_action", env_action=env_action)
        self.command.copy_(env_action).mul_(0.5)
        return self.command

    def observe(self, next_obs, terminated, truncated, final_obs=None):
        self.log.add("observe", next_obs=next_obs, terminated=terminated, truncated=truncated, final_obs=final_obs)
        self.observation[:, :D] = next_obs
        return self.observation


class Normalizer:
    def __init__(self, calls):
        self.calls = calls

    def step(self, obs, reward, terminated, truncated, out):
        self.calls.add("normalizer", obs=obs, reward=reward, terminated=terminated, truncated=truncated, out=out)
        out["reward"].copy_(reward).mul_(0.5)
        torch.bitwise_or(terminated, truncated, out=out["episode_starts"])


class Episodes:
    def __init__(self, calls):
        self.calls = calls

    def step(self, reward, terminated, truncated):
        self.calls.add("episodes", reward=reward, terminated=terminated, truncated=truncated, seen=reward.clone())


class Reward:
    def __init__(self, obs_dim, calls):
        self.num_envs, self.obs_dim, self.act_dim, self.calls, self.reward = N, obs_dim, A, calls, torch.zeros(N)

    def reset(self):
        self.calls.add("reward.reset")

    def step(self, next_obs, action, terminated, truncated, final_obs=None):
        self.calls.add("reward.step", next_obs=next_obs, action=action, terminated=terminated, truncated=truncated, final_obs=final_obs)
        self.reward.copy_(1.0 - next_obs[:, 0].abs())
        return self.reward


def reward_fn(calls):
    """A ``reward_fn`` that logs what it is given and what it returns."""
    def fn(next_obs, info):
        result = 1.0 - next_obs[:, 0].abs()
        calls.add("reward_fn", next_obs=next_obs, info=info, result=result)
        return result

    return fn


class Tally:
    """In `upkie_amd.evaluation.EpisodeTally`'s place."""

    def __init__(self, calls, num_envs, capacity):
        self.calls, self.num_envs, self.capacity = calls, num_envs, capacity

    def reset(self, n_eval_episodes):
        self.calls.add("tally.reset", n_eval_episodes=n_eval_episodes)

    def step(self, reward, terminated, truncated):
        self.calls.add("tally", reward=reward, terminated=terminated, truncated=truncated)


# ---------------------------------------------------------------- host stand-ins for what a driver's file holds
def stage(cls, **attributes):
    obj = cls.__new__(cls)  # (no device: the stage's own class around host tensors)
    vars(obj).update(attributes)
    return obj


def filler(numbers, scale):
    """``f(*shape, dtype=)``: a host tensor filled with the next of ``numbers`` times ``scale``, so that every tensor of
    a set of stand-ins holds its own number and two sets (two scales) differ everywhere."""
    fill = iter(numbers)
    return lambda *shape, dtype=torch.float32: torch.full(shape, next(fill) * scale, dtype=dtype)


def saved_parts(scale, pipeline, reward, stages=()):
    """A stand-in env (2 envs, no persistent observation buffer: the driver supplies its own), an `MlpActorCritic` around
    host tensors, and the keyword arguments of the stages asked for; ``stages`` names further ones (``events``,
    ``targets``, ...) that only hold tensors."""
    from tests.mlp_shapes import dims
    from upkie_amd.policies import MlpActorCritic, mlp_shape

    f = filler(range(100, 200), scale)
    sim = types.SimpleNamespace(state=f(3, 2), reward=f(2), terminated=f(2, dtype=torch.uint8), truncated=f(2, dtype=torch.uint8))
    env = types.SimpleNamespace(num_envs=2, sim=sim, _final_obs=f(2, 4), scale=scale)
    env.state_tensors = lambda: dict(vars(sim), final_obs=env._final_obs)
    shape = mlp_shape(dims(4, [8], 1), dims(4, [8], 1), "tanh", False, 3.0)
    policy = stage(MlpActorCritic, shape=shape, packed=f(6), calls=f(2, dtype=torch.int32), seed=7 * scale, _out={"n": 2})
    kwargs = {}
    if pipeline:
        tensors = {"prev_command": f(2, 1), "observation": f(2, 4), "calls": f(2, dtype=torch.int32)}
        kwargs["pipeline"] = types.SimpleNamespace(num_envs=2, obs_dim=3, act_dim=1, stack=1, frame_dim=4, stacked_dim=4, state_tensors=lambda: tensors)
    if reward:
        terms = {"prev_action": f(1, 2), "term_sum": f(2, 2, dtype=torch.float64), "term_last": f(2, 2, dtype=torch.float64),
                 "finished": f(2, dtype=torch.int32)}
        kwargs["reward"] = types.SimpleNamespace(num_envs=2, obs_dim=3 if pipeline else 4, act_dim=1, state_tensors=lambda: terms)
    for name in stages:
        held = {"calls": f(2, dtype=torch.int32), "observation": f(2, 4)}
        kwargs[name] = types.SimpleNamespace(num_envs=2, dim=3 if pipeline else 4, obs_dim=4, num_targets=0, state_tensors=lambda held=held: held)
    return env, policy, kwargs
