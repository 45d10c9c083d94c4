"""`Ppo`'s rollout step without a GPU: `collect_rollouts()` (``graph=False``) on the CPU oracle env (tests/fake_sim.py)
with recording doubles for the policy, the pipeline, the normaliser, the episode statistics and the reward. For every
configuration: the order of the calls of every step, which tensor OBJECT each call is handed, and the buffer's rows."""

import types

import pytest
import torch

import upkie_amd.envs as envs
from tests.agent_step_doubles import A, D, N, T, Calls, Env, Episodes, Normalizer, Pipeline, Policy, Reward, reward_fn
from tests.fake_sim import oracle_sim_factory
from upkie_amd.exceptions import UpkieRuntimeError
from upkie_amd.ppo import Ppo
from upkie_amd.utils.robot_state import RobotState
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

FIRST_SLOT = 2  # the window starts here, so that the slot wraps inside it: 2, 3, 4, 0, 1


def _model(env, calls, pipeline, normalizer, reward, **kw):
    """A `Ppo` set up by hand as `_setup` would, with the doubles in the stages' places."""
    pipe = Pipeline(calls) if pipeline else None
    words = pipe.stacked_dim if pipeline else D
    if reward == "fn":
        kw["reward_fn"] = reward_fn(calls)
    elif reward == "terms":
        kw["reward"] = Reward(D, calls)
    model = Ppo(env, Policy(words, calls), n_steps=T, pipeline=pipe, normalize=normalizer, graph=False, **kw)
    model.normalizer = Normalizer(calls) if normalizer else None
    model.episodes = Episodes(calls)
    model.buffer = types.SimpleNamespace(
        observations=torch.zeros(T, N, words), actions=torch.zeros(T, N, A), values=torch.zeros(T, N), log_probs=torch.zeros(T, N),
        rewards=torch.zeros(T, N), episode_starts=torch.zeros(T, N, dtype=torch.uint8),
        compute_returns_and_advantage=lambda last_values, dones: calls.add("gae", dones=dones))
    model._env_action = torch.empty(N, A)
    model._starts = torch.ones(N, dtype=torch.uint8)
    model._slot = FIRST_SLOT
    return model


# the calls of ONE step, in order, for every configuration: (pipeline, normaliser, reward) -> names
STEP_CALLS = {
    (False, False, "fn"): ["act", "env.step", "reward_fn", "episodes", "bootstrap"],
    (False, False, "terms"): ["act", "env.step", "reward.step", "episodes", "bootstrap"],
    (False, True, "fn"): ["act", "env.step", "reward_fn", "episodes", "normalizer", "bootstrap"],
    (False, True, "terms"): ["act", "env.step", "reward.step", "episodes", "normalizer", "bootstrap"],
    (True, False, "fn"): ["act", "shape_action", "env.step", "reward_fn", "episodes", "observe", "bootstrap"],
    (True, False, "terms"): ["act", "shape_action", "env.step", "reward.step", "episodes", "observe", "bootstrap"],
    (True, True, "fn"): ["act", "shape_action", "env.step", "reward_fn", "episodes", "observe", "normalizer", "bootstrap"],
    (True, True, "terms"): ["act", "shape_action", "env.step", "reward.step", "episodes", "observe", "normalizer", "bootstrap"],
    (False, False, "env"): ["act", "env.step", "episodes", "bootstrap"],  # neither reward: the env's own
}


@pytest.mark.parametrize("pipeline,normalizer,reward", list(STEP_CALLS))
def test_collect_rollouts_calls_the_stages_in_order_with_the_same_tensors(pipeline, normalizer, reward):
    calls = Calls()
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    inner = envs.make("Upkie-HIP-Pendulum-Vec", num_envs=N, frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=4,
                      sim_factory=oracle_sim_factory)
    with inner:
        model = _model(Env(inner, calls), calls, pipeline, normalizer, reward)
        reset = inner.reset(seed=0)
        model._obs = first_obs = reset[0] if isinstance(reset, tuple) else reset
        pipe, buf, starts, env_action = model.pipeline, model.buffer, model._starts, model._env_action
        model.collect_rollouts()
    assert calls.names == STEP_CALLS[(pipeline, normalizer, reward)] * T + ["value", "gae"]
    assert model._slot == FIRST_SLOT and model.num_timesteps == T * N and (buf.pos, buf.full) == (T, True)
    args = calls.args
    raw_obs = first_obs  # (the raw observation before step k: the reset's, then what the env returned)
    previous_ended = torch.ones(N, dtype=torch.uint8)
    for k in range(T):
        t = (FIRST_SLOT + k) % T
        stepped = args["env.step"][k]
        next_obs, env_reward, terminated, truncated, info = stepped["out"]
        same = dict(terminated=terminated, truncated=truncated)
        # the policy reads the stack with a pipeline, the env's observation without; its outputs are the buffer's slot
        act = args["act"][k]
        assert act["obs"] is (pipe.observation if pipeline else raw_obs)
        assert act["out"]["env_action"] is env_action
        assert {name: x.data_ptr() for name, x in act["out"].items() if name != "env_action"} == dict(
            {"action": buf.actions[t].data_ptr(), "value": buf.values[t].data_ptr(), "log_prob": buf.log_probs[t].data_ptr()},
            **({"norm_obs": buf.observations[t].data_ptr()} if normalizer else {}))
        if not normalizer:
            assert torch.equal(buf.observations[t], act["seen"])
        # the env receives the policy's clamped action, or the command the pipeline shaped from it
        if pipeline:
            assert args["shape_action"][k]["env_action"] is env_action
        applied = pipe.command if pipeline else env_action
        assert stepped["action"] is applied
        # the reward sees the RAW observation and the applied action
        if reward == "fn":
            assert args["reward_fn"][k]["next_obs"] is next_obs and args["reward_fn"][k]["info"] is info
            raw_reward = args["reward_fn"][k]["result"]
        elif reward == "terms":
            given = dict(same, next_obs=next_obs, action=applied, final_obs=info["final_obs"])
            assert all(args["reward.step"][k][name] is x for name, x in given.items())
            raw_reward = model.reward.reward
        else:
            raw_reward = env_reward
        assert args["episodes"][k]["reward"] is raw_reward and all(args["episodes"][k][name] is x for name, x in same.items())
        if pipeline:
            seen = args["observe"][k]
            assert seen["next_obs"] is next_obs and seen["final_obs"] is info["final_obs"] and all(seen[name] is x for name, x in same.items())
        # the normaliser and the bootstrap read the stack and its terminal form with a pipeline
        if normalizer:
            seen = args["normalizer"][k]
            assert seen["obs"] is (pipe.observation if pipeline else next_obs) and seen["reward"] is raw_reward
            assert all(seen[name] is x for name, x in same.items())
            assert set(seen["out"]) == {"reward", "episode_starts"} and seen["out"]["episode_starts"] is starts
            assert seen["out"]["reward"].data_ptr() == buf.rewards[t].data_ptr()
        else:
            assert torch.equal(buf.rewards[t], args["episodes"][k]["seen"]), "without a normaliser the slot holds the raw reward"
            if reward == "env":
                assert torch.equal(buf.rewards[t], stepped["reward"])
        boot = args["bootstrap"][k]
        assert boot["final_obs"] is (pipe.final_observation if pipeline else info["final_obs"]) and all(boot[name] is x for name, x in same.items())
        assert boot["reward"].data_ptr() == buf.rewards[t].data_ptr() and boot["gamma"] == model.gamma
        # the episode starts stored with step k are the ends of step k - 1
        assert torch.equal(buf.episode_starts[t], previous_ended), (k, t)
        previous_ended, raw_obs = stepped["ended"], next_obs
    assert args["env.step"][3]["truncated"].all(), "max_episode_steps = 4: the fourth step truncates every env inside the window"
    assert torch.equal(starts, previous_ended) and args["gae"][0]["dones"] is starts
    assert args["value"][0]["obs"] is (pipe.observation if pipeline else raw_obs)


class _NoFinalObsEnv:
    """An env whose info carries no ``final_obs`` (no same-step autoreset)."""

    num_envs = N

    def __init__(self, calls):
        self.calls = calls

    def step(self, action):
        self.calls.add("env.step", action=action)
        return torch.zeros(N, D), torch.zeros(N), torch.zeros(N, dtype=torch.uint8), torch.zeros(N, dtype=torch.uint8), {}


@pytest.mark.parametrize("pipeline", (False, True))
def test_bootstrap_without_final_obs_raises_in_both_pipeline_settings(pipeline):
    calls = Calls()
    model = _model(_NoFinalObsEnv(calls), calls, pipeline, False, "fn", bootstrap_time_limits=True)
    model._obs = torch.zeros(N, D)
    with pytest.raises(UpkieRuntimeError, match=r"bootstrap_time_limits needs info\['final_obs'\] \(an env with autoreset_mode='same_step'\); "
                                                r"or build Ppo with bootstrap_time_limits=False"):
        model.collect_rollouts()
    assert calls.names == ["act"] + (["shape_action"] if pipeline else []) + ["env.step", "reward_fn", "episodes"]
    assert "bootstrap" not in calls.args and "observe" not in calls.args
    # without the bootstrap the same env steps through
    calls = Calls()
    model = _model(_NoFinalObsEnv(calls), calls, pipeline, False, "fn", bootstrap_time_limits=False)
    model._obs = torch.zeros(N, D)
    model.collect_rollouts()
    assert "bootstrap" not in calls.args and len(calls.args["env.step"]) == T
    if pipeline:
        assert all(seen["final_obs"] is None for seen in calls.args["observe"])
