"""`AgentStep` as its two callers use it, without a GPU: `PolicyEvaluator.begin` / `step` on the CPU oracle env
(tests/fake_sim.py) with the recording doubles of tests/agent_step_doubles.py -- the order of the calls and which tensor
OBJECT each is handed, as tests/test_ppo_rollout_step.py has it for `Ppo` -- and the size checks both constructors share."""

import types

import pytest
import torch

import upkie_amd.envs as envs
import upkie_amd.evaluation as evaluation
from tests.agent_step_doubles import A, D, N, T, Calls, Env, Pipeline, Policy, Reward, Tally, reward_fn
from tests.fake_sim import oracle_sim_factory
from upkie_amd.evaluation import PolicyEvaluator
from upkie_amd.ppo import Ppo
from upkie_amd.utils.robot_state import RobotState
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

E = 7  # episodes asked for (the doubles' tally only records it)


def _evaluator(monkeypatch, inner, calls, pipeline, reward, **kw):
    monkeypatch.setattr(evaluation, "EpisodeTally", lambda num_envs, capacity, device: Tally(calls, num_envs, capacity))
    pipe = Pipeline(calls) if pipeline else None
    if reward == "fn":
        kw["reward_fn"] = reward_fn(calls)
    elif reward == "terms":
        kw["reward"] = Reward(D, calls)
    return PolicyEvaluator(Policy(pipe.stacked_dim if pipeline else D, calls), Env(inner, calls), E, pipeline=pipe, graph=False, **kw)


def _oracle_env():
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    return envs.make("Upkie-HIP-Pendulum-Vec", num_envs=N, frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=4,
                     sim_factory=oracle_sim_factory)


@pytest.mark.parametrize("deterministic", (True, False))
@pytest.mark.parametrize("reward", ("fn", "terms", "env"))
@pytest.mark.parametrize("pipeline", (False, True))
def test_an_evaluation_step_calls_the_stages_in_order_with_the_same_tensors(monkeypatch, pipeline, reward, deterministic):
    calls = Calls()
    with _oracle_env() as inner:
        runner = _evaluator(monkeypatch, inner, calls, pipeline, reward, deterministic=deterministic)
        pipe, action = runner.pipeline, runner._action
        assert (runner.tally.num_envs, runner.tally.capacity, tuple(action.shape)) == (N, E, (N, A))
        runner.begin(E, seed=0)
        # begin: the noise counters zeroed before the pipeline's reset, which follows the env's; then the reward, then the tally
        begun = ((["pipeline.calls.zero_"] if pipeline else []) + ["env.reset"] + (["pipeline.reset"] if pipeline else [])
                 + (["reward.reset"] if reward == "terms" else []) + ["tally.reset"])
        assert calls.names == begun
        assert calls.args["env.reset"][0]["seed"] == 0 and calls.args["tally.reset"][0] == {"n_eval_episodes": E}
        raw_obs = calls.args["env.reset"][0]["out"][0]
        assert raw_obs is inner.observation
        if pipeline:
            assert calls.args["pipeline.reset"][0]["obs"] is raw_obs
        for _ in range(T):
            runner.step()
    acts = "mean_action" if deterministic else "act"
    one_step = ([acts] + (["shape_action"] if pipeline else []) + ["env.step"] + {"fn": ["reward_fn"], "terms": ["reward.step"], "env": []}[reward]
                + (["observe"] if pipeline else []) + ["tally"])
    assert calls.names == begun + one_step * T
    args = calls.args
    for k in range(T):
        stepped = args["env.step"][k]
        next_obs, env_reward, terminated, truncated, info = stepped["out"]
        same = dict(terminated=terminated, truncated=truncated)
        # the policy reads the stack with a pipeline, the env's observation without, and writes the evaluator's action buffer
        act = args[acts][k]
        assert act["obs"] is (pipe.observation if pipeline else raw_obs)
        assert (act["out"] is action) if deterministic else (set(act["out"]) == {"env_action"} and act["out"]["env_action"] is action)
        # the env receives the policy's action, or the command the pipeline shaped from it
        if pipeline:
            assert args["shape_action"][k]["env_action"] is action
        applied = pipe.command if pipeline else action
        assert stepped["action"] is applied
        # the reward sees the RAW observation, the applied action and the terminal observation
        if reward == "fn":
            assert args["reward_fn"][k]["next_obs"] is next_obs and args["reward_fn"][k]["info"] is info
            raw_reward = args["reward_fn"][k]["result"]
        elif reward == "terms":
            given = dict(same, next_obs=next_obs, action=applied, final_obs=info["final_obs"])
            assert all(args["reward.step"][k][name] is x for name, x in given.items())
            raw_reward = runner.reward.reward
        else:
            raw_reward = env_reward
        if pipeline:
            seen = args["observe"][k]
            assert seen["next_obs"] is next_obs and seen["final_obs"] is info["final_obs"] and all(seen[name] is x for name, x in same.items())
        # the tally gets the raw reward and the env's own flags
        assert args["tally"][k]["reward"] is raw_reward and all(args["tally"][k][name] is x for name, x in same.items())
        raw_obs = next_obs
    assert args["env.step"][3]["truncated"].all(), "max_episode_steps = 4: the fourth step truncates every env inside the window"
    assert info["final_obs"] is not None


@pytest.mark.parametrize("pipeline", (False, True))
def test_an_unrecorded_evaluation_step_leaves_only_the_tally_out(monkeypatch, pipeline):
    calls = Calls()
    with _oracle_env() as inner:
        runner = _evaluator(monkeypatch, inner, calls, pipeline, "terms")
        runner.begin(E)
        assert "seed" not in calls.args["env.reset"][0], "without a seed the env is reset plainly"
        del calls.names[:]
        for _ in range(T):
            runner.step(record=False)
    assert calls.names == (["mean_action"] + (["shape_action"] if pipeline else []) + ["env.step", "reward.step"] + (["observe"] if pipeline else [])) * T
    assert "tally" not in calls.args


# ---------------------------------------------------------------- the checks both constructors take from AgentStep
def _sized(num_envs=4, obs_dim=4, act_dim=1, stack=2):
    env = types.SimpleNamespace(num_envs=num_envs, autoreset_mode="same_step", device=torch.device("cpu"))
    frame = obs_dim + act_dim
    pipe = types.SimpleNamespace(num_envs=num_envs, obs_dim=obs_dim, act_dim=act_dim, stack=stack, frame_dim=frame, stacked_dim=stack * frame)
    reward = types.SimpleNamespace(num_envs=num_envs, obs_dim=obs_dim, act_dim=act_dim)
    policy = lambda words: types.SimpleNamespace(shape=types.SimpleNamespace(obs_dim=words, act_dim=act_dim))  # noqa: E731
    return env, policy, pipe, reward


BUILDERS = {"Ppo": lambda env, policy, **kw: Ppo(env, policy, **kw), "PolicyEvaluator": lambda env, policy, **kw: PolicyEvaluator(policy, env, 8, **kw)}


@pytest.mark.parametrize("who", list(BUILDERS))
def test_both_constructors_make_the_same_size_checks(monkeypatch, who):
    monkeypatch.setattr(evaluation, "EpisodeTally", lambda num_envs, capacity, device: Tally(None, num_envs, capacity))
    build = BUILDERS[who]
    env, policy, pipe, reward = _sized()
    # matching sizes: nothing raises, with every combination of the optional stages
    for kw in ({}, {"pipeline": pipe}, {"reward": reward}, {"pipeline": pipe, "reward": reward}, {"reward_fn": lambda obs, info: None}):
        made = build(env, policy(pipe.stacked_dim if "pipeline" in kw else 4), **kw)
        assert made.pipeline is kw.get("pipeline") and made.reward is kw.get("reward") and made.reward_fn is kw.get("reward_fn")
    with pytest.raises(ValueError, match="not both"):
        build(env, policy(4), reward=reward, reward_fn=lambda obs, info: None)
    # the reward against the env, the RAW observation (the pipeline's input, not the stack) and the policy's action
    noun = {"Ppo": "rollout", "PolicyEvaluator": "evaluation"}[who]
    for wrong in ({"num_envs": 8}, {"obs_dim": 5}, {"act_dim": 2}):
        with pytest.raises(ValueError, match=f"the reward serves .* the {noun} has 4, 4 \\(raw\\) and 1"):
            build(env, policy(4), reward=types.SimpleNamespace(**{**vars(reward), **wrong}))
    with pytest.raises(ValueError, match="the reward serves"):
        build(env, policy(pipe.stacked_dim), pipeline=pipe, reward=types.SimpleNamespace(**{**vars(reward), "obs_dim": pipe.stacked_dim}))
    # the pipeline against the policy and the env
    with pytest.raises(ValueError, match="pipeline stacks 2 frames of 5 = 10"):
        build(env, policy(4), pipeline=pipe)
    for wrong in ({"act_dim": 2}, {"num_envs": 8}):
        with pytest.raises(ValueError, match="the pipeline serves"):
            build(env, policy(pipe.stacked_dim), pipeline=types.SimpleNamespace(**{**vars(pipe), **wrong}))
    # what stays the evaluator's own
    if who == "PolicyEvaluator":
        with pytest.raises(ValueError, match="same_step"):
            build(types.SimpleNamespace(**{**vars(env), "autoreset_mode": "next_step"}), policy(4))
        with pytest.raises(ValueError, match="chunk"):
            build(env, policy(4), chunk=0)
