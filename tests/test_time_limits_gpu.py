"""The time-limit bootstrap (MlpActorCritic.bootstrap_time_limits) and the episode statistics (EpisodeStatistics) on the
MI355X: bit for bit against the torch composition and the twins of tests/episodes_reference.py, eager against graph
replay, a Pendulum env with a short time limit, and the example."""

import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import episodes_reference as R
from tests import mlp_reference as M
from tests.mlp_shapes import CASES
from tests.mlp_shapes import policy as _policy
from tests.mlp_shapes import sources_of as _src
from upkie_amd.episodes import EpisodeStatistics
from upkie_amd.graphs import GraphedLoop
from upkie_amd.normalize import RunningNormalizer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GAMMA = 0.99
MASKS = ("none", "one", "sparse", "all")


def _masks(kind, n, seed):
    g = torch.Generator(DEV).manual_seed(seed)
    term = torch.rand(n, device=DEV, generator=g) < 0.2
    if kind == "none":
        trunc = torch.zeros(n, dtype=torch.bool, device=DEV)
    elif kind == "one":
        trunc = torch.zeros(n, dtype=torch.bool, device=DEV)
        trunc[min(n - 1, 16 * (n // 32) + 5)] = True  # one env in one tile
        term[:] = False
    elif kind == "sparse":
        trunc = torch.rand(n, device=DEV, generator=g) < 0.05
    else:
        trunc = torch.ones(n, dtype=torch.bool, device=DEV)
    return term, trunc


def _expected(pol, final_obs, term, trunc, reward):
    gamma_f32 = torch.tensor(GAMMA, dtype=torch.float32, device=DEV)
    v = pol.value(final_obs).clone()
    mask = trunc & ~term
    return torch.where(mask, reward + (gamma_f32 * v), reward), v, mask


def _check_bootstrap(pol, N, D, seed, kinds=MASKS):
    for k, kind in enumerate(kinds):
        g = torch.Generator(DEV).manual_seed(seed + k)
        final_obs = 2.0 * torch.randn(N, D, device=DEV, generator=g)
        reward = torch.randn(N, device=DEV, generator=g)
        term, trunc = _masks(kind, N, seed + 100 + k)
        want, v, mask = _expected(pol, final_obs, term, trunc, reward)
        got = reward.clone()
        as_uint8 = k % 2 == 1  # (bool and uint8 flags)
        ret = pol.bootstrap_time_limits(final_obs, term.to(torch.uint8) if as_uint8 else term, trunc.to(torch.uint8) if as_uint8 else trunc, got, GAMMA)
        assert ret is got
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (kind, (got - want).abs().max().item())
        keep = ~mask
        assert torch.equal(got[keep].view(torch.int32), reward[keep].view(torch.int32)), "masked-out and terminated envs keep their bits"
        if bool((term & trunc).any()):
            both = term & trunc
            assert torch.equal(got[both], reward[both])
        # the fp64 twin of the critic: within fp32 rounding of the policy kernel's own tolerance (1e-5 on the value)
        _, _, v64 = M.forward(pol.shape, _src(pol), final_obs.double().cpu().numpy())
        r64 = reward.double().cpu().numpy()
        m = mask.cpu().numpy()
        twin = np.where(m, r64 + GAMMA * v64, r64)
        assert np.abs(got.double().cpu().numpy() - twin).max() <= 1e-5 * (1.0 + np.abs(twin).max())
        # and the float32 formula of the twin on the kernel's own value
        assert np.array_equal(got.cpu().numpy(), R.bootstrap(reward.cpu().numpy(), v.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), GAMMA))


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}" for c in CASES])
def test_bootstrap_bit_exact(case, normalize):
    N, D, widths, A, act = case
    pol, _, _, _ = _policy(D, widths, A, act, normalize=normalize)
    _check_bootstrap(pol, N, D, seed=11)


@pytest.mark.parametrize("case", [CASES[0], CASES[4]], ids=["4096-4", "1001-5"])
def test_bootstrap_bit_exact_with_a_live_normalizer(case):
    N, D, widths, A, act = case
    pol, _, _, _ = _policy(D, widths, A, act)
    norm = RunningNormalizer(N, D, device=DEV)
    norm.attach(pol)
    g = torch.Generator(DEV).manual_seed(3)
    for _ in range(3):  # the statistics move: the packed obs_mean / obs_std words are live
        norm.step(1.5 * torch.randn(N, D, device=DEV, generator=g) + 0.7, torch.randn(N, device=DEV, generator=g))
    torch.cuda.synchronize()
    assert float(norm.obs_count) > 1.0
    _check_bootstrap(pol, N, D, seed=21)


def test_bootstrap_refuses_bad_arguments():
    N, D, widths, A, act = CASES[1]
    pol, _, _, _ = _policy(D, widths, A, act)
    x = torch.randn(N, D, device=DEV)
    f = torch.zeros(N, dtype=torch.bool, device=DEV)
    r = torch.zeros(N, device=DEV)
    with pytest.raises(ValueError):
        pol.bootstrap_time_limits(x, f, f, r.double(), GAMMA)
    with pytest.raises(ValueError):
        pol.bootstrap_time_limits(x, f, f, torch.zeros(2 * N, device=DEV)[::2], GAMMA)
    with pytest.raises(ValueError):
        pol.bootstrap_time_limits(x, f.float(), f, r, GAMMA)
    with pytest.raises(ValueError):
        pol.bootstrap_time_limits(x, f, f[:-1], r, GAMMA)
    with pytest.raises(ValueError):
        pol.bootstrap_time_limits(x, f, f, r, 1.5)


# ---- episode statistics
def _stream(N, T, period, p_end, seed):
    """A recorded stream: float32 rewards, terminations at random, and truncations every `period` steps for three envs
    in four (synchronised ends: thousands finish in one step) and at other offsets for the rest (scattered ends)."""
    rng = np.random.default_rng(seed)
    rewards = rng.normal(0.5, 1.0, size=(T, N)).astype(np.float32)
    term = rng.random((T, N)) < p_end
    trunc = np.zeros((T, N), dtype=bool)
    offset = np.where(rng.random(N) < 0.25, rng.integers(0, period, N), 0)
    steps = np.arange(T)[:, None]
    trunc[(steps + 1 + offset[None, :]) % period == 0] = True
    return rewards, term, trunc


def _compare(stats, twin):
    ring = stats.ep_info_buffer()
    want = list(twin.ep_info_buffer)
    assert len(ring) == len(want)
    assert [e["l"] for e in ring] == [e["l"] for e in want]
    assert [e["r"] for e in ring] == [e["r"] for e in want], "ring returns bit-equal to sum(Monitor.rewards)"
    assert stats.total_episodes == twin.total_episodes
    means = stats.means.cpu().numpy()
    mr, ml = twin.means()
    assert means[0] == mr and means[1] == ml
    if want:
        assert stats.ep_rew_mean() == mr and stats.ep_len_mean() == ml
        for got, key in ((mr, "r"), (ml, "l")):
            ref = twin.safe_mean(key)
            assert abs(got - ref) <= 1e-12 * max(1.0, abs(ref))
    else:
        assert stats.ep_rew_mean() is None and stats.ep_len_mean() is None
    r, l = twin.running()
    assert np.array_equal(stats.ep_return.cpu().numpy(), r) and np.array_equal(stats.ep_length.cpu().numpy(), l)


@pytest.mark.parametrize("window", [100, 1000])
def test_statistics_bit_equal_to_the_twin_over_a_recorded_stream(window):
    N, T = 4096, 1100
    rewards, term, trunc = _stream(N, T, period=250, p_end=0.002, seed=window)
    stats = EpisodeStatistics(N, window=window, device=DEV)
    twin = R.MonitorTwin(N, window=window)
    d_rew, d_term, d_trunc = (torch.from_numpy(a).to(DEV) for a in (rewards, term, trunc))
    synced = 0
    for t in range(T):
        stats.step(d_rew[t], d_term[t], d_trunc[t].to(torch.uint8))
        twin.step(rewards[t], term[t], trunc[t])
        if t == 3:
            mask = np.arange(N) % 7 == 0  # reset mid-episode: discarded, not recorded
            stats.reset(torch.from_numpy(mask).to(DEV))
            twin.reset(mask)
        if trunc[t].sum() > window:  # (synchronised ends: more finishers than the ring holds)
            synced += 1
        if t % 97 == 0 or t == T - 1 or trunc[t].sum() > window:
            _compare(stats, twin)
    assert synced >= 1 and twin.total_episodes > 2 * N


def test_all_envs_done_in_one_step_keep_the_last_window():
    N = 4096
    stats = EpisodeStatistics(N, window=100, device=DEV)
    reward = torch.arange(N, dtype=torch.float32, device=DEV)
    done = torch.ones(N, dtype=torch.bool, device=DEV)
    stats.step(reward, done, None)
    ring = stats.ep_info_buffer()
    assert [e["r"] for e in ring] == [float(i) for i in range(3996, 4096)]
    assert all(e["l"] == 1 for e in ring)
    assert stats.total_episodes == N
    assert stats.ep_rew_mean() == sum(range(3996, 4096)) / 100
    stats.step(reward, torch.arange(N, device=DEV) == 7, None)  # env 7 ends its new one-step episode: the oldest (3996) leaves
    ring = stats.ep_info_buffer()
    assert ring[0]["r"] == 3997.0 and ring[-1] == {"r": 7.0, "l": 1} and len(ring) == 100


def test_reset_without_a_mask_and_an_empty_ring():
    stats = EpisodeStatistics(37, window=5, device=DEV)
    r = torch.ones(37, device=DEV)
    stats.step(r)
    stats.step(r)
    stats.reset()
    torch.cuda.synchronize()
    assert int(stats.ep_length.abs().sum()) == 0 and stats.total_episodes == 0
    assert stats.ep_rew_mean() is None and stats.ep_info_buffer() == []


# ---- determinism: eager against graph replay
def _graphed_vs_eager():
    N, D, T = 4096, 4, 64
    rewards, term, trunc = _stream(N, T, period=20, p_end=0.01, seed=5)
    d_rew, d_term, d_trunc = (torch.from_numpy(a).to(DEV) for a in (rewards, term, trunc))
    final_obs = torch.randn(T, N, D, device=DEV, generator=torch.Generator(DEV).manual_seed(9))
    runs = []
    for graphed in (False, True):
        pol, _, _, _ = _policy(D, [64, 64], 1, "tanh", normalize=True)
        stats = EpisodeStatistics(N, window=100, device=DEV)
        out = d_rew.clone()
        slot = {"t": 0}

        def body():
            t = slot["t"]
            stats.step(d_rew[t], d_term[t], d_trunc[t])
            pol.bootstrap_time_limits(final_obs[t], d_term[t], d_trunc[t], out[t], GAMMA)
            slot["t"] = (t + 1) % T

        if graphed:
            slot["t"] = T - 1
            loop = GraphedLoop(body, unroll=T, warmup=1)
            for tensor in (stats.ep_return, stats.ep_length, stats.ring_return, stats.ring_length, stats.counters, stats.means):
                tensor.zero_()  # (the warm-up step ran eagerly: start the replay from the same state)
            out.copy_(d_rew)
            loop.replay()
        else:
            for _ in range(T):
                body()
        torch.cuda.synchronize()
        runs.append([t.cpu().clone() for t in (stats.ep_return, stats.ep_length, stats.ring_return, stats.ring_length, stats.counters,
                                               stats.means, out)])
    return runs


def test_graph_replay_is_bit_identical_to_eager_over_two_runs():
    first, second = _graphed_vs_eager(), _graphed_vs_eager()
    for runs in (first, second):
        eager, graphed = runs
        for a, b in zip(eager, graphed):
            assert torch.equal(a.view(torch.uint8) if a.dtype.is_floating_point else a, b.view(torch.uint8) if b.dtype.is_floating_point else b)
    for a, b in zip(first[0], second[0]):
        assert torch.equal(a, b)


# ---- a real env with a short time limit
def test_pendulum_time_limit_lengths():
    import upkie_amd.envs as envs
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    N, limit, T = 1024, 20, 90
    init = RobotState(randomization=RobotStateRandomization(pitch=0.3))
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=N, frequency=200.0, init_state=init, autoreset_mode="same_step",
                   max_episode_steps=limit) as env:
        env.reset(seed=0)
        stats = EpisodeStatistics(N, window=1000, device=env.device)
        g = torch.Generator(env.device).manual_seed(0)
        truncated_seen = fallen_seen = 0
        for _ in range(T):
            before = stats.ep_length.clone()
            action = 2.0 * torch.rand(N, 1, device=env.device, generator=g) - 1.0
            _, reward, terminated, truncated, _ = env.step(action)
            stats.step(reward.float().contiguous(), terminated, truncated)
            by_limit = truncated & ~terminated
            lengths = before + 1
            assert torch.all(lengths[by_limit] == limit), "an episode ended by truncation has exactly max_episode_steps steps"
            assert torch.all(lengths[terminated] <= limit)
            truncated_seen += int(by_limit.sum())
            fallen_seen += int(terminated.sum())
        ring = stats.ep_info_buffer()
        assert ring and all(1 <= e["l"] <= limit for e in ring)
        assert truncated_seen > 0
        assert stats.total_episodes == truncated_seen + fallen_seen


def test_example_prints_the_rollout_statistics():
    env = dict(os.environ, EXAMPLE_STEPS="160")  # 3 x 160 steps: past max_episode_steps = 400, so episodes end
    result = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_mlp_train_time_limits.py")], capture_output=True, text=True,
                            timeout=600, env=env, cwd=os.path.join(ROOT, "examples"))
    assert result.returncode == 0, result.stderr[-3000:]
    lens = [float(x) for x in re.findall(r"ep_len_mean ([0-9.eE+-]+)", result.stdout)]
    rews = [float(x) for x in re.findall(r"ep_rew_mean ([0-9.eE+-]+)", result.stdout)]
    assert lens and rews, result.stdout
    assert all(math.isfinite(x) and 1 <= x <= 400 for x in lens)
    assert all(math.isfinite(x) for x in rews)
    assert "ppo_mlp_train_time_limits:" in result.stdout
