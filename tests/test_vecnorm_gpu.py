"""The running normaliser (upkie_amd.normalize.RunningNormalizer, csrc/vecnorm.hpp) on the MI355X: statistics and
outputs against the fp64 twin of tests/vecnorm_reference.py, the modes, determinism and hipGraph replay, the coupling to
the MLP policy, a closed PPO loop, the example."""

import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import vecnorm_reference as R
from tests.training_rig import reset_pendulum, tower
from upkie_amd.exceptions import UpkieRuntimeError
from upkie_amd.graphs import GraphedLoop
from upkie_amd.normalize import RunningNormalizer, packed_offsets
from upkie_amd.policies import MlpActorCritic
from upkie_amd.rollout import RolloutBuffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _inputs(N, D, T, seed):
    """T steps of float32 obs (column 0: mean 1e3, std 0.1), rewards and about 2 % done envs per step, on the host."""
    rng = np.random.default_rng(seed)
    obs = rng.normal(loc=rng.normal(size=D), scale=rng.uniform(0.5, 3.0, size=D), size=(T, N, D)).astype(np.float32)
    obs[:, :, 0] = rng.normal(loc=1e3, scale=0.1, size=(T, N)).astype(np.float32)
    reward = rng.normal(loc=0.5, scale=2.0, size=(T, N)).astype(np.float32)
    term = (rng.random((T, N)) < 0.01).astype(np.uint8)
    trunc = (rng.random((T, N)) < 0.01).astype(np.uint8)
    return obs, reward, term, trunc


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))), initial=0.0)


def _check_stats(norm, twin):
    mean, var = norm.obs_mean.cpu().numpy(), norm.obs_var.cpu().numpy()
    scale = np.abs(twin.obs_rms.mean) + np.sqrt(twin.obs_rms.var)
    assert np.all(np.abs(mean - twin.obs_rms.mean) <= 1e-9 * scale), np.max(np.abs(mean - twin.obs_rms.mean) / scale)
    assert np.all(np.abs(var - twin.obs_rms.var) <= 1e-9 * twin.obs_rms.var), np.max(np.abs(var - twin.obs_rms.var) / twin.obs_rms.var)
    rm, rv, rc = (float(x) for x in norm.ret_stats.cpu())
    assert abs(rm - twin.ret_rms.mean) <= 1e-9 * (abs(twin.ret_rms.mean) + np.sqrt(twin.ret_rms.var))
    assert abs(rv - twin.ret_rms.var) <= 1e-9 * twin.ret_rms.var
    assert rc == twin.ret_rms.count and float(norm.obs_count) == twin.obs_rms.count
    np.testing.assert_allclose(norm.returns.cpu().numpy(), twin.returns, rtol=1e-12, atol=1e-12)
    m32, s32 = twin.mirrors()
    assert _ulps(norm.obs_mean_f32.cpu().numpy(), m32) <= 1 and _ulps(norm.obs_std_f32.cpu().numpy(), s32) <= 1


CASES = [(4096, 4), (1, 3), (1001, 5), (333, 256), (65536, 30)]


@pytest.mark.parametrize("case", CASES, ids=[f"{n}x{d}" for n, d in CASES])
def test_statistics_and_outputs_against_the_twin(case):
    N, D = case
    T = 200
    obs, reward, term, trunc = _inputs(N, D, T, seed=N + D)
    norm = RunningNormalizer(N, D, device=DEV)
    twin = R.VecNormalizeTwin(N, D)
    d_obs = torch.from_numpy(obs).to(DEV)
    d_rew, d_term, d_trunc = (torch.from_numpy(x).to(DEV) for x in (reward, term, trunc))
    norm_obs = torch.empty(N, D, device=DEV)
    starts = torch.empty(N, dtype=torch.uint8, device=DEV)
    norm.reset(d_obs[T - 1])
    twin.reset(obs[T - 1])
    for t in range(T):
        r = norm.step(d_obs[t], d_rew[t], d_term[t], d_trunc[t].bool(), out={"norm_obs": norm_obs, "episode_starts": starts})
        want_obs, want_r, want_starts = twin.step(obs[t], reward[t], term[t], trunc[t])
        assert _ulps(r.cpu().numpy(), want_r) <= 1, t
        np.testing.assert_array_equal(starts.cpu().numpy(), want_starts)
        np.testing.assert_allclose(norm_obs.cpu().numpy(), want_obs, rtol=2e-6, atol=2e-6)
        if t % 20 == 0 or t == T - 1:
            _check_stats(norm, twin)
    # normalised observations: (u - m) / sd in fp32 with the device's own mirrors, clipped -- bit for bit
    m, s = norm.obs_mean_f32.cpu().numpy(), norm.obs_std_f32.cpu().numpy()
    want = np.clip((obs[T - 1] - m) / s, np.float32(-10.0), np.float32(10.0))
    np.testing.assert_array_equal(norm.normalize_obs(d_obs[T - 1]).cpu().numpy(), want)
    assert int(norm.workspace[:4].cpu().view(torch.int32)) == 0, "the ticket is back at zero"


def test_modes():
    N, D = 1000, 6
    obs, reward, term, trunc = _inputs(N, D, 3, seed=5)
    o, r, te, tr = (torch.from_numpy(x[0]).to(DEV) for x in (obs, reward, term, trunc))
    warm = RunningNormalizer(N, D, device=DEV)
    warm.step(torch.from_numpy(obs[1]).to(DEV), torch.from_numpy(reward[1]).to(DEV))
    sd = warm.state_dict()

    frozen = RunningNormalizer(N, D, training=False, device=DEV)
    frozen.load_state_dict(sd)
    frozen.training = False
    before = (frozen.obs_stats.clone(), frozen.ret_stats.clone(), frozen.returns.clone())
    got = frozen.step(o, r, te, tr).cpu().numpy()
    assert torch.equal(frozen.obs_stats, before[0]) and torch.equal(frozen.ret_stats, before[1])
    twin = R.VecNormalizeTwin(N, D)
    twin.ret_rms.var = float(sd["ret_var"])
    assert _ulps(got, twin.normalize_reward(reward[0])) <= 1
    done = (term[0] | trunc[0]).astype(bool)
    np.testing.assert_array_equal(frozen.returns.cpu().numpy(), np.where(done, 0.0, before[2].cpu().numpy()))

    raw = RunningNormalizer(N, D, norm_reward=False, device=DEV)
    got = raw.step(o, r, te, tr)
    assert torch.equal(got, r)
    assert float(raw.ret_count) == pytest.approx(N + 1e-4) and float(raw.obs_count) == pytest.approx(N + 1e-4)

    no_obs = RunningNormalizer(N, D, norm_obs=False, device=DEV)
    no_obs.reset(o)
    no_obs.step(o, r, te, tr)
    assert float(no_obs.obs_count) == 1e-4 and torch.equal(no_obs.obs_var, torch.ones(D, dtype=torch.float64, device=DEV))
    assert float(no_obs.ret_count) == pytest.approx(N + 1e-4)
    assert torch.equal(no_obs.normalize_obs(o), o)

    assert bool((raw.returns != 0).any())
    raw.reset(o)
    assert int((raw.returns != 0).sum()) == 0
    assert float(raw.obs_count) == pytest.approx(2 * N + 1e-4), "reset updates the observation statistics"


def _run_steps(norm, data, outs, order):
    """Steps with the inputs of slots `order`, writing the slots' outputs (reward, norm_obs or None, episode_starts)."""
    d_obs, d_rew, d_term, d_trunc = data
    for t in order:
        out = {"reward": outs[0][t], "episode_starts": outs[2][t]}
        if outs[1] is not None:
            out["norm_obs"] = outs[1][t]
        norm.step(d_obs[t], d_rew[t], d_term[t], d_trunc[t], out=out)


@pytest.mark.parametrize("two_launch", [True, False], ids=["two-launch", "one-launch"])
def test_determinism_and_graph_replay(two_launch):
    N, D, T = 4096, 4, 50
    obs, reward, term, trunc = _inputs(N, D, T, seed=11)
    data = [torch.from_numpy(x).to(DEV) for x in (obs, reward, term, trunc)]

    def fresh():
        norm = RunningNormalizer(N, D, norm_reward=two_launch, device=DEV)
        outs = (torch.zeros(T, N, device=DEV), torch.zeros(T, N, D, device=DEV) if two_launch else None,
                torch.zeros(T, N, dtype=torch.uint8, device=DEV))
        return norm, outs

    def snapshot(norm, outs):
        return [x.clone() for x in (norm.obs_stats, norm.ret_stats, norm.returns, norm.obs_mean_f32, norm.obs_std_f32) + tuple(o for o in outs if o is not None)]

    order = [(i + 1) % T for i in range(T)]  # (the slot order of a capture that follows one warm-up step)
    runs = []
    for _ in range(2):
        norm, outs = fresh()
        _run_steps(norm, data, outs, order)
        first = snapshot(norm, outs)
        _run_steps(norm, data, outs, order)
        runs.append((first, snapshot(norm, outs)))
    for a, b in zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1]):
        assert torch.equal(a, b)

    norm, outs = fresh()
    state = [norm.obs_stats, norm.ret_stats, norm.returns, norm.obs_mean_f32, norm.obs_std_f32]
    saved = [x.clone() for x in state]
    slot = {"t": 0}

    def body():
        t = slot["t"]
        _run_steps(norm, data, outs, [t])
        slot["t"] = (t + 1) % T

    loop = GraphedLoop(body, unroll=T, warmup=1)
    for x, s in zip(state, saved):
        x.copy_(s)
    for want in runs[0]:
        loop.replay()
        torch.cuda.synchronize()
        for a, b in zip(snapshot(norm, outs), want):
            assert torch.equal(a, b)
    assert int(norm.workspace[:4].cpu().view(torch.int32)) == 0


def test_policy_coupling():
    N, D = 1001, 5
    torch.manual_seed(2)
    actor, critic = tower(D, 2, 64).to(DEV), tower(D, 1, 64).to(DEV)
    log_std = nn.Parameter(torch.zeros(2, device=DEV))
    policy = MlpActorCritic.from_modules(actor, critic, log_std, [-1.0, -1.0], [1.0, 1.0])
    norm = RunningNormalizer(N, D, clip_obs=3.0, device=DEV)
    with pytest.raises(ValueError, match="observation words"):
        RunningNormalizer(N, D + 1, device=DEV).attach(policy)
    norm.attach(policy)
    assert policy.shape.normalize == 1 and policy.shape.clip_obs == 3.0
    obs, reward, term, trunc = _inputs(N, D, 6, seed=3)
    data = [torch.from_numpy(x).to(DEV) for x in (obs, reward, term, trunc)]
    mine, theirs = torch.empty(N, D, device=DEV), torch.empty(N, D, device=DEV)
    for t in range(5):
        norm.step(data[0][t], data[1][t], data[2][t], data[3][t], out={"norm_obs": mine})
        policy.act(data[0][t], deterministic=True, out={"norm_obs": theirs})
        assert torch.equal(mine, theirs), t
        m, s = policy.unpack()[0:2]
        assert torch.equal(m, norm.obs_mean_f32) and torch.equal(s, norm.obs_std_f32)
    policy.act(data[0][5], deterministic=True, out={"norm_obs": theirs})
    assert torch.equal(norm.normalize_obs(data[0][5]), theirs)
    # an optimiser step and update_from re-pack the weights, not stale statistics
    opt = torch.optim.SGD(list(actor.parameters()) + list(critic.parameters()) + [log_std], lr=0.1)
    loss = actor(mine).pow(2).mean() + critic(mine).pow(2).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    policy.update_from()
    m, s = policy.unpack()[0:2]
    assert torch.equal(m, norm.obs_mean_f32) and torch.equal(s, norm.obs_std_f32)
    assert not torch.equal(norm.obs_mean_f32, torch.zeros(D, device=DEV))
    mean_at, std_at = packed_offsets(D)
    assert torch.equal(policy.packed[std_at: std_at + D], norm.obs_std_f32)
    with pytest.raises(UpkieRuntimeError, match="first call"):
        RunningNormalizer(N, D, device=DEV).attach(policy)  # (already called)


def test_closed_loop_eager_against_the_twin_and_graphed_bit_equal():
    N, T = 4096, 128
    results = []
    for graphed in (False, True):
        torch.manual_seed(0)
        with reset_pendulum(N) as env:
            dev = env.device
            actor, critic = tower(4, 1, 64).to(dev), tower(4, 1, 64).to(dev)
            policy = MlpActorCritic.from_modules(actor, critic, nn.Parameter(torch.zeros(1, device=dev)), [-1.0], [1.0], seed=0)
            norm = RunningNormalizer.for_env(env)
            norm.attach(policy)
            buf = RolloutBuffer(T, N, obs_shape=(4,), action_shape=(1,), device=dev)
            obs = env.observation
            env_action = torch.empty(N, 1, device=dev)
            starts = torch.ones(N, dtype=torch.uint8, device=dev)
            norm.reset(obs)
            twin = R.VecNormalizeTwin(N, 4)
            twin.reset(obs.cpu().numpy())
            slot, last = {"t": 0}, {}

            def body():
                t = slot["t"]
                buf.episode_starts[t].copy_(starts)
                out = policy.act(obs, out={"norm_obs": buf.observations[t], "action": buf.actions[t], "value": buf.values[t],
                                           "log_prob": buf.log_probs[t], "env_action": env_action})
                next_obs, reward, terminated, truncated, _ = env.step(out[0])
                norm.step(next_obs, reward, terminated, truncated, out={"reward": buf.rewards[t], "episode_starts": starts})
                last["step"] = (next_obs, reward, terminated, truncated)
                slot["t"] = (t + 1) % T

            keep = list(env.state_tensors().values())  # (`obs` among them)
            keep += [norm.obs_stats, norm.ret_stats, norm.returns, norm.obs_mean_f32, norm.obs_std_f32, policy.packed, starts]
            saved = [x.clone() for x in keep]
            if graphed:
                loop = GraphedLoop(body, unroll=T, warmup=1)
                for x, s in zip(keep, saved):
                    x.copy_(s)
                policy.reseed()
                loop.replay()
            else:
                slot["t"] = 1  # (the slot order of the capture)
                allocated = None
                for i in range(T):
                    t = slot["t"]
                    body()
                    if i == 2:
                        gc.collect()  # (cyclic garbage of earlier tests holds device memory until a collection: not during the count)
                        torch.cuda.synchronize()
                        allocated = torch.cuda.memory_allocated(dev)
                    o, r, te, tr = (x.cpu().numpy() for x in last["step"])
                    _, want_r, _ = twin.step(o, r, te, tr)
                    assert _ulps(buf.rewards[t].cpu().numpy(), want_r) <= 1
                    if i % 16 == 0 or i == T - 1:
                        _check_stats(norm, twin)
                torch.cuda.synchronize()
                assert torch.cuda.memory_allocated(dev) == allocated, "a warm step allocates nothing"
            torch.cuda.synchronize()
            results.append([buf.observations.clone(), buf.actions.clone(), buf.values.clone(), buf.rewards.clone(), buf.episode_starts.clone(),
                            norm.obs_stats.clone(), norm.ret_stats.clone(), norm.returns.clone(), policy.packed.clone()])
    for eager, graph in zip(*results):
        assert torch.equal(eager, graph)


def test_rollout_buffer_add_policy_step_allocates_nothing():
    N, T = 1000, 4
    torch.manual_seed(1)
    actor, critic = tower(6, 2, 64).to(DEV), tower(6, 1, 64).to(DEV)
    policy = MlpActorCritic.from_modules(actor, critic, nn.Parameter(torch.zeros(2, device=DEV)), [-1.0, -1.0], [1.0, 1.0])
    norm = RunningNormalizer(N, 6, device=DEV)
    norm.attach(policy)
    buf = RolloutBuffer(T, N, obs_shape=(6,), action_shape=(2,), device=DEV)
    obs, reward, term, trunc = (torch.from_numpy(x).to(DEV) for x in _inputs(N, 6, T + 1, seed=4))
    starts = torch.zeros(N, dtype=torch.uint8, device=DEV)
    out = policy.act(obs[0])
    norm.step(obs[0], reward[0], term[0], trunc[0], out={"episode_starts": starts})
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated(DEV)
    for t in range(T):
        out = policy.act(obs[t], out={"norm_obs": buf.observations[t], "action": buf.actions[t], "value": buf.values[t], "log_prob": buf.log_probs[t]})
        r = norm.step(obs[t + 1], reward[t + 1], term[t + 1], trunc[t + 1], out={"reward": buf.rewards[t]})
        buf.add_policy_step(None, r, starts, out)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(DEV) == allocated
    assert buf.full


def test_example_runs():
    env = dict(os.environ, EXAMPLE_STEPS="16")
    result = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_mlp_normalized_rollout.py")], capture_output=True, text=True,
                            timeout=600, env=env, cwd=os.path.join(ROOT, "examples"))
    assert result.returncode == 0, result.stderr[-3000:]
    assert "ppo_mlp_normalized_rollout:" in result.stdout
