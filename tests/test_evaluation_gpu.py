"""The evaluation tally on the MI355X against the fp64 twin of SB3's ``evaluate_policy`` loop (tests/
evaluation_reference.py), bit for bit: alone over scripted streams at every grid geometry, after a reset and under graph
replay; `evaluate_policy` on a real env, graphed and eager; `MlpActorCritic.mean_action`; and a training run with an
`EvalCallback` against the same run without."""

import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import evaluation_reference as R
from tests.training_rig import pendulum, pitch_reward, same, tower
from upkie_amd import evaluation
from upkie_amd.evaluation import EpisodeTally, EvalCallback, evaluate_policy
from upkie_amd.exceptions import UpkieRuntimeError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


# ---------------------------------------------------------------- the tally alone
def _device_script(script):
    return tuple(torch.from_numpy(a.copy()).to(DEV) for a in (script.rewards, script.terminated, script.truncated))  # (the script is read-only)


def _state(tally):
    """Everything the tally holds, on the host, with the records cut at `filled`."""
    filled, steps = tally.counters.cpu().tolist()
    return {"filled": filled, "steps": steps, "rec_return": tally.rec_return[:filled].cpu().numpy(), "rec_length": tally.rec_length[:filled].cpu().numpy(),
            "rec_env": tally.rec_env[:filled].cpu().numpy(), "rec_truncated": tally.rec_truncated[:filled].cpu().numpy(),
            "count": tally.count.cpu().numpy(), "target": tally.target.cpu().numpy(), "ep_return": tally.ep_return.cpu().numpy(),
            "ep_length": tally.ep_length.cpu().numpy(), "summary": tally.summary.cpu().numpy()}


def _same_state(a, b):
    return a.keys() == b.keys() and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def _compare(tally, twin, where):
    got = _state(tally)
    k = twin.filled
    assert got["filled"] == k and got["steps"] == twin.steps, where
    assert np.array_equal(got["rec_return"], np.array(twin.rec_return, dtype=np.float64)), where  # (the same bits: == on fp64)
    assert np.array_equal(got["rec_length"], np.array(twin.rec_length, dtype=np.int32)), where
    assert np.array_equal(got["rec_env"], np.array(twin.rec_env, dtype=np.int32)), where
    assert np.array_equal(got["rec_truncated"], np.array(twin.rec_truncated, dtype=np.uint8)), where
    assert np.array_equal(got["count"], twin.count) and np.array_equal(got["target"], twin.target), where
    ret, length = twin.running()
    assert np.array_equal(got["ep_return"], ret) and np.array_equal(got["ep_length"], length), where
    if k == twin.E:
        assert got["summary"].tolist() == list(twin.summary()), where
    else:
        assert not got["summary"].any(), f"{where}: the summary is written by the step that fills the list, not before"


@pytest.mark.parametrize("row", R.EVAL_ROWS, ids=R.EVAL_IDS)
def test_the_tally_is_the_twin_bit_for_bit_after_every_step(row):
    script = R.eval_script(row)
    rewards, term, trunc = _device_script(script)
    twin = R.evaluate_twin(row.N, row.E)
    tally = EpisodeTally(row.N, row.E, device=DEV)
    tally.reset(row.E)
    assert tally.remaining() == row.E
    for t in range(R.EVAL_STEPS):
        twin.step(script.rewards[t], script.terminated[t], script.truncated[t])
        tally.step(rewards[t], term[t], trunc[t])
        _compare(tally, twin, f"step {t}")
        assert tally.remaining() == row.E - twin.filled
    assert twin.filled == row.E, "the script fills the quota"
    result = tally.result()
    mean_r, var_r, mean_l, var_l, lo, hi, frac = twin.summary()
    assert result["mean_reward"] == mean_r and result["std_reward"] == math.sqrt(var_r)
    assert result["mean_ep_length"] == mean_l and result["std_ep_length"] == math.sqrt(var_l)
    assert (result["min_reward"], result["max_reward"], result["time_limit_frac"]) == (lo, hi, frac)
    assert result["episode_rewards"] == list(twin.rec_return) and result["episode_lengths"] == list(twin.rec_length)
    assert result["episode_envs"] == list(twin.rec_env)
    print(f"N {row.N} E {row.E}: full after {twin.steps} steps, mean {mean_r:.6g} std {math.sqrt(var_r):.6g} time limits {frac:.3f}")


def test_a_larger_capacity_and_missing_flags_change_nothing():
    row = R.EvalRow(257, 300, "")
    script = R.eval_script(row)
    rewards, term, trunc = _device_script(script)
    twin = R.EvaluateTwin(row.N, row.E)
    tally = EpisodeTally(row.N, 1000, device=DEV)
    tally.reset(row.E)
    for t in range(R.EVAL_STEPS):
        none_term, none_trunc = not script.terminated[t].any(), not script.truncated[t].any()
        twin.step(script.rewards[t], script.terminated[t], script.truncated[t])
        tally.step(rewards[t], None if none_term else term[t].view(torch.uint8), None if none_trunc else trunc[t])
        _compare(tally, twin, f"step {t}")
    assert any(not script.terminated[t].any() for t in range(R.EVAL_STEPS))
    with pytest.raises(ValueError):
        tally.reset(1001)
    with pytest.raises(UpkieRuntimeError):
        EpisodeTally(4, 4, device=DEV).step(rewards[0, :4])


def test_reset_starts_clean():
    row = R.EvalRow(4099, 1025, "")
    script = R.eval_script(row)
    rewards, term, trunc = _device_script(script)
    used = EpisodeTally(row.N, row.E, device=DEV)
    used.reset(row.E)
    for t in range(R.EVAL_STEPS):
        used.step(rewards[t], term[t], trunc[t])
    assert used.remaining() == 0
    E2 = 777
    fresh = EpisodeTally(row.N, row.E, device=DEV)
    fresh.reset(E2)
    used.reset(E2)
    assert _same_state(_state(used), _state(fresh)) and used.remaining() == E2
    twin = R.EvaluateTwin(row.N, E2)
    for t in range(R.EVAL_STEPS):
        for tally in (used, fresh):
            tally.step(rewards[t], term[t], trunc[t])
        twin.step(script.rewards[t], script.terminated[t], script.truncated[t])
        assert _same_state(_state(used), _state(fresh)), t
        _compare(used, twin, f"step {t} after the reset")
    assert twin.filled == E2 and used.result() == fresh.result()


def test_the_tally_under_graph_replay_gives_the_eager_bits():
    from upkie_amd.graphs import GraphedLoop

    row = R.EvalRow(65537, 70000, "")
    script = R.eval_script(row)
    rewards, term, trunc = _device_script(script)
    T = R.EVAL_STEPS
    eager = EpisodeTally(row.N, row.E, device=DEV)
    eager.reset(row.E)
    for t in range(T):
        eager.step(rewards[t], term[t], trunc[t])
    want = _state(eager)
    assert want["filled"] == row.E
    tally = EpisodeTally(row.N, row.E, device=DEV)
    tally.reset(row.E)
    slot = {"t": T - 1}  # (the capture's warm-up step takes the last slot)

    def body():
        t = slot["t"]
        tally.step(rewards[t], term[t], trunc[t])
        slot["t"] = (t + 1) % T

    loop = GraphedLoop(body, unroll=T, warmup=1, device=DEV)
    for replay in range(2):
        tally.reset(row.E)
        loop.replay()
        torch.cuda.synchronize()
        assert _same_state(_state(tally), want), f"replay {replay}"
    loop.replay()  # a full list: twelve more steps change nothing
    torch.cuda.synchronize()
    assert _same_state(_state(tally), want)


# ---------------------------------------------------------------- evaluate_policy on a real env
def _env(num_envs=64, mode="same_step", limit=20, **kw):
    import upkie_amd.envs as envs
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    init = RobotState(randomization=RobotStateRandomization(pitch=0.3))
    # (fall_pitch below the widest initial pitch: some episodes end by a fall, at once or within the 20 steps, the others by the time limit)
    return envs.make("Upkie-HIP-Pendulum-Vec", num_envs=num_envs, frequency=200.0, init_state=init, autoreset_mode=mode, max_episode_steps=limit,
                     fall_pitch=0.25, **kw)


def _policy(obs_dim=4, low=-1.0, high=1.0, seed=0):
    from upkie_amd.policies import MlpActorCritic

    torch.manual_seed(3)
    actor, critic = tower(obs_dim, 1).to(DEV), tower(obs_dim, 1).to(DEV)
    return MlpActorCritic.from_modules(actor, critic, nn.Parameter(torch.zeros(1, device=DEV)), action_low=[low], action_high=[high], seed=seed)


class _Recorded:
    """`EpisodeTally.step` wrapped to keep what every step hands the tally (eager runs only: it copies to the host)."""

    def __init__(self, monkeypatch):
        self.steps = []
        inner = EpisodeTally.step

        def step(tally, reward, terminated=None, truncated=None):
            self.steps.append((reward.cpu().numpy().copy(), terminated.cpu().numpy().copy(), truncated.cpu().numpy().copy()))
            return inner(tally, reward, terminated, truncated)

        monkeypatch.setattr(EpisodeTally, "step", step)
        self.undo = monkeypatch.undo

    def twin(self, N, E):
        twin = R.EvaluateTwin(N, E)
        for reward, term, trunc in self.steps:
            twin.step(reward, term, trunc)
        return twin


def _run(E=100, **kw):
    """One whole evaluation in fresh objects: `EpisodeTally.result`'s dict."""
    with _env() as env:
        runner = evaluation.PolicyEvaluator(_policy(), env, E, reward_fn=pitch_reward, chunk=kw.pop("chunk", 32), graph=kw.pop("graph", True))
        return runner.run(E, seed=kw.pop("seed", 5), **kw)


def test_evaluate_policy_on_a_real_env_is_the_twin_graphed_and_eager(monkeypatch):
    N, E, limit = 64, 100, 20
    recorded = _Recorded(monkeypatch)
    eager = _run(graph=False)
    recorded.undo()
    twin = recorded.twin(N, E)
    assert twin.filled == E and twin.steps <= len(recorded.steps) <= 2 * limit, "two episodes of 20 steps at the most"
    lengths, rewards = eager["episode_lengths"], eager["episode_rewards"]
    assert rewards == list(twin.rec_return) and lengths == list(twin.rec_length) and eager["episode_envs"] == list(twin.rec_env)
    mean_r, var_r, mean_l, var_l, lo, hi, frac = twin.summary()
    assert (eager["mean_reward"], eager["std_reward"], eager["mean_ep_length"]) == (mean_r, math.sqrt(var_r), mean_l)
    assert max(lengths) <= limit and min(lengths) >= 1
    by_limit = [bool(t) for t in twin.rec_truncated]
    assert all(length == limit for length, t in zip(lengths, by_limit) if t), "a time limit ends an episode at max_episode_steps"
    assert eager["time_limit_frac"] == frac == sum(by_limit) / E
    print(f"lengths {min(lengths)}-{max(lengths)}, time_limit_frac {frac}, mean reward {mean_r:.6g} +/- {math.sqrt(var_r):.6g}")
    assert 0.0 < frac < 1.0, "the fixture ends episodes both ways"
    assert sorted(set(eager["episode_envs"])) == list(range(N)) and np.bincount(eager["episode_envs"]).tolist() == R.targets(N, E).tolist()
    graphed = _run(graph=True)
    assert graphed == eager, "graphed and eager evaluations from one seed"
    assert _run(graph=True, chunk=1) == eager and _run(graph=False, chunk=1) == eager, "chunk = 1 and chunk = 32"
    assert _run(graph=True, seed=6)["episode_rewards"] != rewards, "another seed, other episodes"
    # the public function: SB3's two return forms
    with _env() as env:
        policy = _policy()
        assert evaluate_policy(policy, env, n_eval_episodes=E, reward_fn=pitch_reward, seed=5) == (mean_r, math.sqrt(var_r))
        assert evaluate_policy(policy, env, n_eval_episodes=E, reward_fn=pitch_reward, seed=5, return_episode_rewards=True) == (rewards, lengths)
        own = evaluate_policy(policy, env, n_eval_episodes=E, seed=5, return_episode_rewards=True)  # the env's own reward: the reference's constant 0
        assert own == ([0.0] * E, lengths)


def test_evaluate_policy_with_a_pipeline_and_reward_terms(monkeypatch):
    from upkie_amd.pipeline import AgentPipeline
    from upkie_amd.rewards import RewardTerms, Term, act_rate, obs, one, terminated

    N, E, K = 64, 100, 3
    terms = lambda: {"alive": Term(1.0, taps=[one()]), "upright": Term(-1.0, "abs", taps=[obs(0)]),  # noqa: E731
                     "action_rate": Term(-0.01, "square", taps=[act_rate(0)]), "fall": Term(-10.0, taps=[terminated()])}

    def run(graph):
        with _env() as env:
            pipe = AgentPipeline(N, 4, [-1.0], [1.0], dt=1.0 / 200.0, stack=K, integrate_action=True, action_noise=[0.02], action_lag=0.05,
                                 observation_noise=[0.002, 0.002, 0.01, 0.01], seed=0, device=env.device)
            reward = RewardTerms(N, 4, 1, dt=1.0 / 200.0, terms=terms(), device=env.device)
            policy = _policy(obs_dim=pipe.stacked_dim, low=-2.0, high=2.0)
            runner = evaluation.PolicyEvaluator(policy, env, E, pipeline=pipe, reward=reward, graph=graph)
            first = runner.run(E, seed=5)
            return first, runner.run(E, seed=5)

    recorded = _Recorded(monkeypatch)
    eager, again = run(False)
    recorded.undo()
    assert again == eager, "a second evaluation from the same seed in the same objects"
    half = len(recorded.steps) // 2
    twin = R.EvaluateTwin(N, E)
    for reward, term, trunc in recorded.steps[:half]:
        twin.step(reward, term, trunc)
    assert twin.filled == E
    assert eager["episode_rewards"] == list(twin.rec_return) and eager["episode_lengths"] == list(twin.rec_length)
    assert min(eager["episode_rewards"]) < -5.0, "a fall's penalty, computed on the terminal observation, is in the raw reward"
    graphed, graphed_again = run(True)
    assert graphed == eager and graphed_again == eager


def test_mean_action_is_the_deterministic_act_and_touches_nothing():
    policy = _policy()
    torch.manual_seed(1)
    obs = torch.randn(64, 4, device=DEV)
    policy.act(obs)  # (a sampled call: the buffers and the counters exist and have moved)
    env_action = policy.act(obs, deterministic=True)[0].clone()
    before = [policy.calls.clone()] + [policy._out[k].clone() for k in ("env_action", "action", "value", "log_prob")]
    out = torch.full((64, 1), 7.0, device=DEV)
    assert policy.mean_action(obs, out) is out and torch.equal(out, env_action)
    other = torch.randn(1000, 4, device=DEV)
    big = torch.full((1000, 1), 7.0, device=DEV)
    policy.mean_action(other, big)
    assert torch.equal(big[:64], policy.mean_action(other[:64].contiguous(), torch.empty(64, 1, device=DEV))), "a row does not depend on the batch"
    assert bool((big.abs() <= 1.0).all()) and bool((big != 7.0).all())
    after = [policy.calls] + [policy._out[k] for k in ("env_action", "action", "value", "log_prob")]
    for a, b in zip(after, before):
        assert torch.equal(a, b)
    fresh = _policy()
    fresh.mean_action(other, big)
    assert fresh.calls is None and fresh._out == {}, "nothing is allocated either"
    with pytest.raises(ValueError):
        policy.mean_action(obs, torch.empty(63, 1, device=DEV))


def test_a_sampled_evaluation_runs_at_the_policys_batch_size_and_advances_its_counters():
    E = 100
    with _env() as env:
        policy = _policy()
        sampled = evaluate_policy(policy, env, n_eval_episodes=E, deterministic=False, reward_fn=pitch_reward, seed=5, graph=False, return_episode_rewards=True)
        calls = policy.calls.clone()
        assert len(sampled[0]) == E and max(sampled[1]) <= 20
        assert int(calls.min()) >= max(sampled[1]) and int(calls.min()) == int(calls.max()), "one draw per env per step taken"
        mean = evaluate_policy(policy, env, n_eval_episodes=E, reward_fn=pitch_reward, seed=5, graph=False, return_episode_rewards=True)
        assert torch.equal(policy.calls, calls), "the deterministic evaluation draws nothing"
        assert mean[0] != sampled[0], "the noise is in the actions"
    with _env(num_envs=32) as env:
        with pytest.raises(ValueError, match="batches of 64"):
            evaluate_policy(policy, env, n_eval_episodes=E, deterministic=False, seed=5, graph=False)


# ---------------------------------------------------------------- training is untouched
def _learn(tmp_path, with_callback):
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.ppo import Ppo

    B, n_steps = 256, 32  # the smallest case of tests/test_ppo_learn_gpu.py: its env, its policy, its arguments
    torch.manual_seed(0)
    env = pendulum(B, 40, pitch=0.1)
    dev = env.device
    policy = MlpActorCritic.from_modules(tower(4, 1, 64).to(dev), tower(4, 1, 64).to(dev), nn.Parameter(torch.zeros(1, device=dev)), action_low=[-1.0],
                                         action_high=[1.0], seed=0)
    kw = dict(n_steps=n_steps, n_epochs=3, batch_size=B * n_steps // 4, reward_fn=pitch_reward, seed=0)
    with env, _env(num_envs=96, limit=40) as eval_env:
        # iterations end at vec-env steps 32, 64, 96: evaluations behind the second and the third
        callback = EvalCallback(eval_env, n_eval_episodes=150, eval_freq=40, best_model_save_path=str(tmp_path / "best.pt"), seed=9) if with_callback else None
        model = Ppo(env, policy, **kw).learn(3 * B * n_steps, callback=callback)
        torch.cuda.synchronize()
        tr, nz = model.trainer, model.normalizer
        tensors = [policy.packed, tr.m, tr.v, tr.control, tr.stats, policy.calls, model._obs] + [v for _, v in sorted(model.episodes.state_tensors().items())]
        tensors = [t.clone() for t in tensors]
        return tensors, nz.state_dict(), model.records, callback


def test_a_run_with_an_eval_callback_trains_bit_for_bit_as_one_without(tmp_path):
    plain, plain_norm, plain_records, _ = _learn(tmp_path, False)
    evald, evald_norm, evald_records, callback = _learn(tmp_path, True)
    for a, b in zip(evald, plain):
        assert torch.equal(a, b)

    assert same(evald_norm, plain_norm), "the normaliser's statistics"
    assert len(evald_records) == len(plain_records) == 3
    for k, (a, b) in enumerate(zip(evald_records, plain_records)):
        assert same({key: v for key, v in a.items() if not key.startswith("eval/")}, b), "train/*, rollout/* and time/*"
        assert [key for key in a if key.startswith("eval/")] == ([] if k == 0 else ["eval/mean_reward", "eval/mean_ep_length", "eval/time_limit_frac"])
    assert callback.evaluations["timesteps"] == [2 * 256 * 32, 3 * 256 * 32]
    assert [len(r) for r in callback.evaluations["results"]] == [150, 150]
    assert callback.last_mean_reward == evald_records[2]["eval/mean_reward"]
    assert callback.best_mean_reward == max(evald_records[1]["eval/mean_reward"], evald_records[2]["eval/mean_reward"])
    assert os.path.exists(tmp_path / "best.pt")
    print("eval records:", [{k: v for k, v in rec.items() if k.startswith("eval/")} for rec in evald_records])


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("mode", ["next_step", "disabled"])
def test_evaluation_refuses_an_env_without_same_step_autoreset(mode):
    with _env(mode=mode) as env:
        with pytest.raises(ValueError, match="same_step"):
            evaluate_policy(_policy(), env, n_eval_episodes=10)


def test_evaluation_refuses_to_run_without_a_bound_and_says_when_the_quota_is_not_met():
    with _env(limit=None) as env:
        with pytest.raises(ValueError, match="max_steps"):
            evaluate_policy(_policy(), env, n_eval_episodes=10)
    import upkie_amd.envs as envs

    # envs that start upright and cannot fall within two steps: no episode is shorter than the time limit's 20
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=64, frequency=200.0, autoreset_mode="same_step", max_episode_steps=20) as env:
        for graph in (False, True):
            with pytest.raises(UpkieRuntimeError, match="0 of 10 episodes"):
                evaluate_policy(_policy(), env, n_eval_episodes=10, max_steps=2, graph=graph, chunk=2)
        with pytest.raises(UpkieRuntimeError, match="0 of 10 episodes"):
            evaluate_policy(_policy(), env, n_eval_episodes=10, max_steps=19, seed=0)
        assert evaluate_policy(_policy(), env, n_eval_episodes=10, max_steps=20, seed=0, return_episode_rewards=True)[1] == [20] * 10


# ---------------------------------------------------------------- the example
def test_the_evaluation_example_runs():
    env = dict(os.environ, EXAMPLE_STEPS="16")
    result = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_learn_eval.py")], capture_output=True, text=True, timeout=600, env=env,
                            cwd=os.path.join(ROOT, "examples"))
    assert result.returncode == 0, result.stderr[-3000:]
    lines = [ln for ln in result.stdout.splitlines() if ln.startswith("iteration")]
    assert len(lines) == 4 and all("train/loss" in ln for ln in lines), result.stdout
    assert ["eval/mean_reward" in ln for ln in lines] == [False, True, False, True], result.stdout
    assert "evaluate_policy:" in result.stdout and "best eval/mean_reward" in result.stdout
