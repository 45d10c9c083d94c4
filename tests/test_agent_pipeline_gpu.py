"""The agent pipeline on the MI355X against its numpy twin (tests/agent_pipeline_reference.py): data movement bit for
bit, the arithmetic one step at a time from the device's own state under derived bounds, graph replay against the
eager run, and `Ppo(pipeline=...)`: the buffer's rows, finite logs, save / load, the example."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import agent_pipeline_reference as P
from tests.agent_pipeline_shapes import _dev, _np
from tests.training_rig import pendulum, tower
from upkie_amd.pipeline import AgentPipeline
from upkie_amd.ppo import Ppo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32 = np.float32
EPS = 2.0 ** -24


# ---------------------------------------------------------------- data movement
@pytest.mark.parametrize("with_final", [True, False])
@pytest.mark.parametrize("K, D, A", [(1, 4, 1), (8, 4, 1), (4, 36, 6), (3, 79, 6)])  # (3, 79, 6): 255 of the 256-word cap
def test_data_movement_is_bit_exact(K, D, A, with_final):
    """No noise, no lag, no integration: `observation`, `final_observation` and `command` are the twin's bits over 3 K
    steps of a batch in which about a tenth of the envs end per step (scripted masks), with one masked `reset` on the
    way. N is no multiple of the envs a wavefront serves."""
    N = 777
    rng = np.random.default_rng(K * 1000 + D)
    low, high = [-1.0] * A, [1.0] * A
    pipe = AgentPipeline(N, D, low, high, 0.005, stack=K, device=DEV)
    twins = [P.Twin(e, D, low, high, 0.005, stack=K) for e in range(N)]
    S = pipe.stacked_dim
    assert S == K * (D + A)
    first = rng.normal(size=(N, D)).astype(F32)
    got = pipe.reset(_dev(first))
    want = np.stack([tw.reset(first[e]).copy() for e, tw in enumerate(twins)])
    assert np.array_equal(_np(got), want)
    want_final = np.zeros((N, S), dtype=F32)
    for t in range(3 * K):
        action = rng.uniform(-1, 1, size=(N, A)).astype(F32)
        nxt, fin = rng.normal(size=(N, D)).astype(F32), rng.normal(size=(N, D)).astype(F32)
        term, trunc = rng.uniform(size=N) < 0.05, rng.uniform(size=N) < 0.05
        done = term | trunc
        cmd = pipe.shape_action(_dev(action))
        obs = pipe.observe(_dev(nxt), _dev(term), _dev(trunc.astype(np.uint8)), final_obs=_dev(fin) if with_final else None)
        want_cmd, want_obs = P.run_batch(twins, action, nxt, done, fin if with_final else None)
        assert np.array_equal(_np(cmd), want_cmd) and np.array_equal(want_cmd, action)
        assert np.array_equal(_np(obs), want_obs), t
        assert obs.data_ptr() == pipe.observation.data_ptr()
        if with_final:
            for e in np.nonzero(done)[0]:
                want_final[e] = twins[e].final.reshape(-1)
        assert np.array_equal(_np(pipe.final_observation), want_final), "rows of envs that did not end keep what they held"
        want_prev = np.stack([tw.prev_command for tw in twins])
        assert np.array_equal(_np(pipe.prev_command), want_prev)
        if t == K:  # a masked reset on the way: the others keep their state
            mask = rng.uniform(size=N) < 0.3
            again = rng.normal(size=(N, D)).astype(F32)
            got = pipe.reset(_dev(again), _dev(mask))
            for e in np.nonzero(mask)[0]:
                twins[e].reset(again[e])
            assert np.array_equal(_np(got), np.stack([tw.stack.reshape(-1) for tw in twins]))
            assert np.array_equal(_np(pipe.prev_command), np.stack([tw.prev_command for tw in twins]))
    assert not pipe.calls.any(), "no noise: the counters do not move"


# ---------------------------------------------------------------- arithmetic, one step at a time
@pytest.mark.parametrize("noise", [False, True])
def test_arithmetic_one_step_at_a_time_from_the_devices_own_state(noise):
    """Every step starts from the DEVICE's prev_command and counters, so errors do not accumulate. Each stage is at most
    three float32 roundings of values bounded by m = max(|low|, |high|, 1): |device - twin| <= 4 * 2^-24 * m per
    command word without noise. With noise a draw is held to the twin's by the bound of the policy's draws
    (1e-6 + 2e-7 |z|, tests/test_mlp_policy_gpu.py) times sigma, added to it (the clip is 1-Lipschitz). A noised
    observation column is one fma, one rounding of a value v on the device and one in the twin's store:
    2 * 2^-24 * max(|v|, 1) plus the draw's bound times sigma."""
    N, D, A, K = 515, 6, 3, 4
    rng = np.random.default_rng(5 + noise)
    low, high = [-1.0, -3.0, -0.25], [1.0, 2.0, 0.5]
    m = np.maximum(np.maximum(np.abs(low), np.abs(high)), 1.0)
    sig_a, sig_o = ([0.05, 0.3, 0.0] if noise else None), ([0.01, 0.0, 0.1, 0.02, 0.5, 0.003] if noise else None)
    kw = dict(stack=K, integrate_action=True, action_noise=sig_a, action_lag=0.03, observation_noise=sig_o, seed=(7 << 32) | 12345)
    pipe = AgentPipeline(N, D, low, high, 0.01, device=DEV, **kw)
    twins = [P.Twin(e, D, low, high, 0.01, **kw) for e in range(N)]
    pipe.reset(_dev(rng.normal(size=(N, D)).astype(F32)))
    worst, worst_obs = 0.0, 0.0
    for t in range(24):
        scale = 100.0 if t % 6 == 5 else 1.0  # (every sixth step drives the integrator into its bounds)
        action = (rng.uniform(-1, 1, size=(N, A)) * m * scale).astype(F32)
        prev, calls = _np(pipe.prev_command).copy(), _np(pipe.calls).astype(np.int64) & 0xFFFFFFFF
        cmd = _np(pipe.shape_action(_dev(action)))
        for e, tw in enumerate(twins):
            exact, z = tw.shape_action_exact(action[e], prev=prev[e], call=calls[e])
            bound = 4 * EPS * m
            if noise:
                bound = bound + np.asarray(sig_a) * (1e-6 + 2e-7 * np.abs(z))
            err = np.abs(cmd[e].astype(np.float64) - exact)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (t, e, err, bound)
        assert np.array_equal(_np(pipe.prev_command), cmd)
        assert np.array_equal(_np(pipe.calls).astype(np.int64) & 0xFFFFFFFF, calls + (1 if noise else 0))
        # the observation: the shift is a copy (bit for bit), the new frame's columns under the bound above
        before, calls = _np(pipe.observation).copy().reshape(N, K, -1), _np(pipe.calls).astype(np.int64) & 0xFFFFFFFF
        nxt = rng.normal(size=(N, D)).astype(F32)
        done = rng.uniform(size=N) < 0.1
        obs = _np(pipe.observe(_dev(nxt), _dev(done), None, final_obs=_dev(nxt))).reshape(N, K, -1)
        for e in range(N):
            if done[e]:
                assert not obs[e, :-1].any() and not obs[e, -1, D:].any()
            else:
                assert np.array_equal(obs[e, :-1], before[e, 1:]) and np.array_equal(obs[e, -1, D:], cmd[e])
            x = nxt[e].astype(np.float64)
            bound = 2 * EPS * np.maximum(np.abs(x), 1.0)
            if noise:
                z = np.array([P.philox_normal(e, int(calls[e]), d >> 2, d & 3, pipe.seed) for d in range(D)])
                x = x + np.asarray(sig_o, dtype=F32).astype(np.float64) * z
                bound = 2 * EPS * np.maximum(np.abs(x), 1.0) + np.asarray(sig_o) * (1e-6 + 2e-7 * np.abs(z))
            err = np.abs(obs[e, -1, :D].astype(np.float64) - x)
            worst_obs = max(worst_obs, float((err / bound).max()))
            assert (err <= bound).all(), (t, e, err, bound)
    print(f"noise {noise}: worst command error / bound {worst:.3f}, worst observation error / bound {worst_obs:.3f}")
    # a poisoned action word: the neutral command, prev_command kept
    prev = pipe.prev_command.clone()
    action = torch.zeros(N, A, device=DEV)
    action[3, 1], action[4, 0] = float("nan"), float("inf")
    cmd = pipe.shape_action(action)
    assert cmd[3, 1] == 0 and cmd[4, 0] == 0 and pipe.prev_command[3, 1] == prev[3, 1] and pipe.prev_command[4, 0] == prev[4, 0]
    assert torch.isfinite(cmd).all() and torch.isfinite(pipe.prev_command).all()


# ---------------------------------------------------------------- with an env and a policy
def _reward(next_obs, info):
    return torch.abs(next_obs[:, 1]).mul_(-0.25).sub_(torch.abs(next_obs[:, 0])).add_(1.0)


def _make(B, K=8, noise=True, shaped=True, limit=40):
    from upkie_amd.policies import MlpActorCritic

    torch.manual_seed(0)
    env = pendulum(B, limit, pitch=0.1)
    dev = env.device
    pipe = AgentPipeline(B, 4, [-1.0], [1.0], 1.0 / 200.0, stack=K, integrate_action=shaped, action_lag=0.05 if shaped else None,
                         action_noise=[0.02] if noise else None, observation_noise=[0.002, 0.002, 0.01, 0.01] if noise else None, seed=3,
                         device=dev)
    D = pipe.stacked_dim
    actor, critic = tower(D, 1, 64).to(dev), tower(D, 1, 64).to(dev)
    log_std = nn.Parameter(torch.zeros(1, device=dev))
    bound = 2.0 if shaped else 1.0
    policy = MlpActorCritic.from_modules(actor, critic, log_std, action_low=[-bound], action_high=[bound], seed=0)
    return env, policy, pipe


def test_a_graphed_rollout_step_with_the_pipeline_replays_the_eager_bits():
    from upkie_amd.graphs import GraphedLoop

    B, unroll, replays = 256, 4, 3
    results = []
    for graphed in (False, True):
        env, policy, pipe = _make(B)
        with env:
            env.reset(seed=0)
            obs = env.observation
            pipe.reset(obs)
            env_action = torch.empty(B, 1, device=env.device)

            def step():
                policy.act(pipe.observation, out={"env_action": env_action})
                next_obs, _, terminated, truncated, info = env.step(pipe.shape_action(env_action))
                pipe.observe(next_obs, terminated, truncated, final_obs=info["final_obs"])

            if graphed:
                loop = GraphedLoop(step, unroll=unroll, warmup=1, device=env.device)
                for _ in range(replays):
                    loop.replay()
            else:
                for _ in range(1 + unroll * replays):
                    step()
            torch.cuda.synchronize()
            results.append([t.clone() for t in (pipe.observation, pipe.final_observation, pipe.command, pipe.prev_command, pipe.calls, obs)])
    for a, b in zip(*results):
        assert torch.equal(a, b)
    assert int(results[0][4].min()) == 1 + 2 * (1 + unroll * replays), "one draw per env at reset, two per step"


def test_ppo_with_a_pipeline_learns_and_its_buffer_holds_the_twins_stack():
    B, T, K = 256, 16, 8
    env, policy, pipe = _make(B, K=K)
    with env:
        model = Ppo(env, policy, n_steps=T, n_epochs=3, batch_size=B * T // 4, reward_fn=_reward, seed=0, pipeline=pipe).learn(2 * B * T)
        torch.cuda.synchronize()
        assert model.iterations == 2 and len(model.records) == 2
        assert model.normalizer.obs_dim == K * 5 and model.buffer.observations.shape == (T, B, K * 5)
        for rec in model.records:
            values = {k: v for k, v in rec.items() if k.startswith("train/") and isinstance(v, float)}
            assert len(values) >= 7 and all(np.isfinite(v) for v in values.values()), rec
        assert (pipe.calls > 0).all() and pipe.observation.abs().sum() > 0
    # no noise, no shaping, no normaliser, eager: the buffer's rows are the twin's stack of the recorded raw observations
    env, policy, pipe = _make(B, K=K, noise=False, shaped=False, limit=6)
    raw = []

    def recording_reward(next_obs, info):
        raw.append((next_obs.clone(), info["final_obs"].clone()))
        return _reward(next_obs, info)

    with env:
        model = Ppo(env, policy, n_steps=T, n_epochs=1, batch_size=B * T, reward_fn=recording_reward, seed=0, pipeline=pipe, normalize=False,
                    graph=False)
        model._setup()
        first = _np(model._obs)
        model.learn(B * T)
        torch.cuda.synchronize()
        buf = model.buffer
        rows, actions, starts = _np(buf.observations), _np(buf.actions), _np(buf.episode_starts)
        last_starts, last_obs = _np(model._starts), _np(pipe.observation)
    assert len(raw) == T
    twins = [P.Twin(e, 4, [-1.0], [1.0], 1.0 / 200.0, stack=K) for e in range(B)]
    want = np.stack([tw.reset(first[e]).copy() for e, tw in enumerate(twins)])
    ended = 0
    for t in range(T):
        assert np.array_equal(rows[t], want), t
        done = (starts[t + 1] if t + 1 < T else last_starts) != 0
        ended += int(done.sum())
        nxt, fin = _np(raw[t][0]), _np(raw[t][1])
        _, want = P.run_batch(twins, np.clip(actions[t], -1.0, 1.0), nxt, done, fin)
    assert np.array_equal(last_obs, want) and ended >= 2 * B, "the time limit of 6 steps ended every env twice"


def test_ppo_with_a_pipeline_resumes_bit_for_bit(tmp_path):
    """tests/test_ppo_learn_gpu.py's save / load test with a pipeline, noise on: 4 iterations in one run equal 2, save,
    load into fresh objects, 2 more."""
    B, T = 256, 16
    per = B * T
    sched = dict(learning_rate=lambda p: 1e-3 * p, clip_range=lambda p: 0.1 + 0.2 * p, target_kl=0.05)

    def driver():
        env, policy, pipe = _make(B)
        return env, policy, dict(n_steps=T, n_epochs=3, batch_size=per // 4, reward_fn=_reward, seed=0, pipeline=pipe, **sched)

    env, policy, kw = driver()
    with env:
        whole = Ppo(env, policy, **kw).learn(4 * per)
        torch.cuda.synchronize()
        want, want_records = policy.packed.clone(), whole.records
        want_state = [t.clone() for t in kw["pipeline"].state_tensors().values()]
    path = str(tmp_path / "ppo.pt")
    env, policy, kw = driver()
    with env:
        first = Ppo(env, policy, **kw).learn(4 * per, callback=lambda m, rec: m.iterations < 2)
        assert first.iterations == 2
        first.save(path)
    env, policy, kw = driver()
    with env:
        resumed = Ppo.load(path, env, policy, **kw)
        assert resumed.iterations == 2 and resumed.num_timesteps == 2 * per
        resumed.learn(2 * per, reset_num_timesteps=False)
        torch.cuda.synchronize()
        assert torch.equal(policy.packed, want), "2 + save + load + 2 iterations equal 4 iterations, bit for bit"
        for a, b in zip(kw["pipeline"].state_tensors().values(), want_state):
            assert torch.equal(a, b)
        for a, b in zip(resumed.records, want_records[2:]):
            assert a.keys() == b.keys()
            for key in a:
                assert a[key] == b[key] or (a[key] != a[key] and b[key] != b[key]), key
    # a file saved without a pipeline is refused
    env, policy, kw = driver()
    sd = torch.load(path, map_location="cpu", weights_only=True)
    sd["tensors"] = {k: v for k, v in sd["tensors"].items() if not k.startswith("pipeline.")}
    bare = str(tmp_path / "bare.pt")
    torch.save(sd, bare)
    with env:
        with pytest.raises(ValueError, match="pipeline"):
            Ppo.load(bare, env, policy, **kw)


def test_pipeline_example_runs():
    env = dict(os.environ, EXAMPLE_STEPS="16")
    result = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_learn_pipeline.py")], capture_output=True, text=True, timeout=600,
                            env=env, cwd=os.path.join(ROOT, "examples"))
    assert result.returncode == 0, result.stderr[-3000:]
    lines = [ln for ln in result.stdout.splitlines() if ln.startswith("iteration")]
    assert len(lines) >= 2, result.stdout
    for ln in lines:
        words = ln.replace(",", " ").split()
        values = [float(words[i + 1]) for i, w in enumerate(words[:-1]) if w.startswith("train/") and w not in ("train/early_stopped_at",)]
        assert len(values) >= 7 and all(np.isfinite(v) for v in values), ln
