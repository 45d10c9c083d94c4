"""PPO.learn's pieces on the MI355X: the target_kl early stop against the fp64 twin (tests/ppo_learn_reference.py) and
against a trainer stopped by construction, the controlled entry points against the uncontrolled ones, schedules and a
stop under graph replay, the explained variance, two data-parallel ranks, and the `Ppo` driver against the hand-written
loop of examples/ppo_mlp_train_time_limits.py, with save / load."""

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import ppo_learn_reference as L
from tests.mlp_shapes import CASES, T
from tests.mlp_shapes import restore_trainer as _restore
from tests.mlp_shapes import trainer_case as _setup
from tests.mlp_shapes import trainer_state as _state
from tests.training_rig import np64, pendulum, pitch_reward, tower
from upkie_amd.ppo import STAT_NAMES, Ppo, PpoTrainer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = CASES[0]  # 4096 envs, obs 4, [64, 64] tanh, one action: 8192 samples
TOTAL = T * CASE[0]
MB = TOTAL // 4


def _data(buf, case):
    flat = lambda t: np64(t).reshape(-1)  # noqa: E731
    return dict(obs=np64(buf.observations).reshape(-1, case[1]), actions=np64(buf.actions).reshape(-1, case[3]), old_values=flat(buf.values),
                old_log_prob=flat(buf.log_probs), advantages=flat(buf.advantages), returns=flat(buf.returns))


def _all(pol, tr):
    return _state(pol, tr) + [tr.stats.clone()]


def test_early_stop_lands_where_sb3s_does():
    lr = 1e-2
    pol, _, _, _, buf = _setup(CASE, seed=1, first=True)
    tr = PpoTrainer(pol, lr=lr, n_epochs=4, batch_size=MB, seed=5, controlled=True)
    tr.prepare(buf)
    perms = [tr.perm[e].long().cpu().numpy() for e in range(4)]
    src0 = [np64(s) for s in pol.sources()]
    data = _data(buf, CASE)
    free = L.train(pol.shape, src0, data, perms, MB, lr=lr)
    kls = free["rows"][:, 4]
    print("twin approx_kl without a stop:", kls)
    chosen = L.choose_target_kl(kls)
    assert chosen is not None, "the inputs give the twin a gap of a factor four in approx_kl"
    target_kl, k = chosen
    twin = L.train(pol.shape, src0, data, perms, MB, lr=lr, target_kl=target_kl)
    assert twin["stopped_at"] == divmod(k, 4) and 0 < k < 15
    threshold = 1.5 * target_kl
    assert all(x <= threshold / 2 or x >= 2 * threshold for x in twin["rows"][:, 4]), "every approx_kl a factor of two from the threshold"
    tr.set_target_kl(target_kl)
    stats = tr.update(buf, sync=False)
    rec = tr.log()
    torch.cuda.synchronize()
    rows = stats.double().cpu().numpy().reshape(16, 7)
    print("device approx_kl:", rows[:, 4], "stop", rec["early_stopped_at"], "twin", twin["stopped_at"])
    assert rec["early_stopped_at"] == twin["stopped_at"]
    np.testing.assert_allclose(rows[:k + 1][:, [0, 1, 3, 6]], twin["rows"][:, [0, 1, 3, 6]], rtol=2e-3, atol=2e-5)
    assert np.isnan(rows[k + 1:]).all() and not np.isnan(rows[:k + 1]).any()
    ctrl = tr.control.cpu().numpy()
    assert ctrl[1] == k == twin["applied"], "t counts the minibatches applied"
    assert rec["n_updates"] == twin["n_updates"] == tr.state_dict()["n_updates"] and ctrl[5] == 1.0 and ctrl[7] == k + 1
    for name in STAT_NAMES[:4] + STAT_NAMES[6:]:
        assert rec[name] == pytest.approx(twin["record"][name], rel=2e-3, abs=2e-5), name
    assert abs(rec["approx_kl"] - twin["record"]["approx_kl"]) <= 1e-4
    # a second trainer stopped by construction after k minibatches: e whole epochs, then j minibatches of epoch e
    e, j = divmod(k, 4)
    pol2, _, _, _, buf2 = _setup(CASE, seed=1, first=True)
    tr2 = PpoTrainer(pol2, lr=lr, n_epochs=4, batch_size=MB, seed=5)
    tr2.prepare(buf2)
    assert torch.equal(tr2.perm, tr.perm)
    if e:
        tr2.n_epochs = e
        tr2.update(buf2, sync=False)
    if j:
        tr2.perm[0].copy_(tr.perm[e])
        tr2.n_epochs, tr2.n_minibatches = 1, j
        tr2.update(buf2, sync=False)
    torch.cuda.synchronize()
    for a, b in zip(_state(pol, tr), _state(pol2, tr2)):
        assert torch.equal(a, b), "weights, m, v, (lr, t): those after the last minibatch that ran, bit for bit"


@pytest.mark.parametrize("target_kl", [None, 1e9])
def test_a_target_kl_that_never_fires_gives_the_uncontrolled_bits(target_kl):
    kw = dict(n_epochs=2, batch_size=(TOTAL + 2) // 3, seed=1, ent_coef=0.003, clip_range_vf=0.3)
    pol, _, _, _, buf = _setup(CASE, seed=3)
    plain = PpoTrainer(pol, **kw)
    assert not plain.controlled
    plain.train(buf, sync=False)
    want = _all(pol, plain)
    pol2, _, _, _, buf2 = _setup(CASE, seed=3)
    tr = PpoTrainer(pol2, target_kl=target_kl, controlled=True, **kw)
    tr.train(buf2, sync=False)
    torch.cuda.synchronize()
    for a, b in zip(_all(pol2, tr), want):
        assert torch.equal(a, b)
    rec = tr.log()
    assert rec["early_stopped_at"] is None and rec["n_updates"] == 2 == plain.log()["n_updates"]


def test_schedules_under_capture():
    pol, _, _, _, buf = _setup(CASE, seed=3)
    kw = dict(n_epochs=2, batch_size=MB, seed=2)
    tr = PpoTrainer(pol, clip_range=lambda p: 0.3 * p, lr=lambda p: 3e-4 * p, **kw)
    tr.prepare(buf)
    s0 = _state(pol, tr)
    tr.update(buf, sync=False)  # warm-up
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr.update(buf, sync=False)
    fractions = []
    for progress in (1.0, 0.5, 0.1):
        _restore(pol, tr, s0)
        tr.set_progress(progress)
        graph.replay()
        torch.cuda.synchronize()
        got = _all(pol, tr)
        rec = tr.log()
        assert rec["clip_range"] == 0.3 * progress and rec["learning_rate"] == 3e-4 * progress
        pol2, _, _, _, buf2 = _setup(CASE, seed=3)
        eager = PpoTrainer(pol2, clip_range=0.3 * progress, lr=3e-4 * progress, **kw)
        eager.train(buf2, sync=False)
        torch.cuda.synchronize()
        assert torch.equal(eager.perm, tr.perm)
        for a, b in zip(got, _all(pol2, eager)):
            assert torch.equal(a, b), progress
        fractions.append(rec["clip_fraction"])
    print("clip fractions:", fractions)
    assert fractions[0] < fractions[1] < fractions[2]


def test_a_captured_update_survives_a_stop():
    pol, _, _, _, buf = _setup(CASE, seed=3)  # (old log-probs perturbed: approx_kl is about 0.03 from the first minibatch)
    kw = dict(n_epochs=2, batch_size=MB, seed=4)
    tr = PpoTrainer(pol, target_kl=1e-4, **kw)
    tr.prepare(buf)
    s0 = _state(pol, tr)
    graph = torch.cuda.CUDAGraph()
    tr.update(buf, sync=False)
    with torch.cuda.graph(graph):
        tr.update(buf, sync=False)
    _restore(pol, tr, s0)
    graph.replay()
    rec = tr.log()
    assert rec["early_stopped_at"] == (0, 0)
    for a, b in zip(_state(pol, tr)[:3], s0[:3]):
        assert torch.equal(a, b), "stopped at the first minibatch: nothing moved"
    assert torch.isnan(tr.stats.reshape(-1, 7)[1:]).all() and not torch.isnan(tr.stats[0, 0]).any()
    tr.set_target_kl(None)
    graph.replay()
    torch.cuda.synchronize()
    got = _all(pol, tr)
    assert tr.log()["early_stopped_at"] is None
    pol2, _, _, _, buf2 = _setup(CASE, seed=3)
    eager = PpoTrainer(pol2, **kw)
    eager.train(buf2, sync=False)
    torch.cuda.synchronize()
    for a, b in zip(got, _all(pol2, eager)):
        assert torch.equal(a, b), "the re-armed replay is a full update"


def test_explained_variance_against_numpy_fp64():
    pol, _, _, _, buf = _setup(CASE, seed=2)
    tr = PpoTrainer(pol, n_epochs=1, batch_size=MB)
    tr.prepare(buf)
    a = tr.explained_variance().clone()
    b = tr.explained_variance().clone()
    want = L.explained_variance(np64(buf.values), np64(buf.returns))
    print("explained variance:", float(a), "numpy fp64:", want, "difference:", abs(float(a) - want))
    assert abs(float(a) - want) <= 1e-6
    assert a.view(torch.int64).item() == b.view(torch.int64).item(), "the same bits on two calls"
    buf.returns = torch.full_like(buf.returns, 1.25)
    tr.prepare(buf)
    assert math.isnan(float(tr.explained_variance()))
    # an odd count, not a multiple of the block
    pol3, _, _, _, buf3 = _setup(CASES[4], seed=2)
    tr3 = PpoTrainer(pol3, n_epochs=1, batch_size=500)
    tr3.train(buf3)
    rec = tr3.log()
    assert abs(rec["explained_variance"] - L.explained_variance(np64(buf3.values), np64(buf3.returns))) <= 1e-6
    assert rec["std"] == pytest.approx(float(np.exp(np64(pol3.sources()[4])).mean()), rel=1e-6)


def test_two_gloo_ranks_stop_at_the_same_minibatch(tmp_path):
    out = str(tmp_path / "stop")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           "29761", os.path.join(ROOT, "tests", "ppo_learn_distributed_worker.py"), out]
    result = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, OMP_NUM_THREADS="1"), cwd=ROOT)
    assert result.returncode == 0, result.stderr[-3000:]
    res = []
    for rank in range(2):
        with open(f"{out}.{rank}") as f:
            res.append(json.load(f))
    print(res)
    for r in res:
        assert r["chosen"], "the union's approx_kl sequence has a gap of a factor four"
        assert r["stopped_at"] == r["union_stopped_at"] == r["expected"] and r["stopped_at"] is not None
        assert r["ranks_bit_equal"] == [True] * 6, r["ranks_bit_equal"]
        assert r["t"] == r["union_t"] and r["n_updates"] == r["union_n_updates"]
        assert r["nan_after"] and r["rows_close"]
    assert res[0]["stopped_at"] == res[1]["stopped_at"]


# ---------------------------------------------------------------- the driver
def _make(B):
    from upkie_amd.policies import MlpActorCritic

    torch.manual_seed(0)
    env = pendulum(B, 40, pitch=0.1)
    dev = env.device
    actor, critic = tower(4, 1, 64).to(dev), tower(4, 1, 64).to(dev)
    log_std = nn.Parameter(torch.zeros(1, device=dev))
    policy = MlpActorCritic.from_modules(actor, critic, log_std, action_low=[-1.0], action_high=[1.0], seed=0)
    return env, policy


def _hand_written_loop(B, n_steps, iterations):
    """examples/ppo_mlp_train_time_limits.py's loop, verbatim but for the sizes."""
    from upkie_amd.episodes import EpisodeStatistics
    from upkie_amd.graphs import GraphedLoop
    from upkie_amd.normalize import RunningNormalizer
    from upkie_amd.rollout import RolloutBuffer

    env, policy = _make(B)
    with env:
        dev = env.device
        normalizer = RunningNormalizer.for_env(env, gamma=0.99)
        normalizer.attach(policy)
        episodes = EpisodeStatistics(B, window=100, device=dev)
        trainer = PpoTrainer(policy, n_epochs=3, batch_size=B * n_steps // 4, obs_normalized=True, seed=0)
        buffer = RolloutBuffer(n_steps, B, obs_shape=(4,), action_shape=(1,), device=dev)
        env.reset(seed=0)
        obs = env.observation
        normalizer.reset(obs)
        env_action = torch.empty(B, 1, device=dev)
        reward = torch.empty(B, device=dev)
        starts = torch.ones(B, dtype=torch.uint8, device=dev)
        slot = {"t": n_steps - 1}

        def rollout_step():
            t = slot["t"]
            buffer.episode_starts[t].copy_(starts)
            out = policy.act(obs, out={"norm_obs": buffer.observations[t], "action": buffer.actions[t], "value": buffer.values[t],
                                       "log_prob": buffer.log_probs[t], "env_action": env_action})
            next_obs, _, terminated, truncated, info = env.step(out[0])
            torch.abs(next_obs[:, 0], out=reward).neg_().add_(1.0)
            episodes.step(reward, terminated, truncated)
            normalizer.step(next_obs, reward, terminated, truncated, out={"reward": buffer.rewards[t], "episode_starts": starts})
            policy.bootstrap_time_limits(info["final_obs"], terminated, truncated, buffer.rewards[t], buffer.gamma)
            slot["t"] = (t + 1) % n_steps

        loop = GraphedLoop(rollout_step, unroll=n_steps, warmup=1)
        records = []
        for _ in range(iterations):
            loop.replay()
            buffer.pos, buffer.full = n_steps, True
            buffer.compute_returns_and_advantage(last_values=policy.value(obs), dones=starts)
            stats = trainer.train(buffer)
            records.append((stats.clone(), episodes.ep_rew_mean(), episodes.ep_len_mean()))
        torch.cuda.synchronize()
        return policy.packed.clone(), records


def _driver(B, n_steps, **kw):
    env, policy = _make(B)
    return env, policy, dict(n_steps=n_steps, n_epochs=3, batch_size=B * n_steps // 4, reward_fn=pitch_reward, seed=0, **kw)


def test_learn_equals_the_hand_written_loop_and_resumes_bit_for_bit(tmp_path):
    B, n_steps = 256, 32
    packed, records = _hand_written_loop(B, n_steps, 3)
    env, policy, kw = _driver(B, n_steps)
    with env:
        model = Ppo(env, policy, **kw).learn(3 * B * n_steps)
        torch.cuda.synchronize()
        assert model.iterations == 3 and model.num_timesteps == 3 * B * n_steps
        assert torch.equal(policy.packed, packed), "packed weights bit for bit"
        assert len(model.records) == 3
        for rec, (stats, rew, length) in zip(model.records, records):
            rows = stats.double().cpu().numpy().reshape(-1, 7)
            for k, name in enumerate(STAT_NAMES):
                assert rec[f"train/{name}"] == float(rows[:, k].mean()), name
            assert rec["rollout/ep_rew_mean"] == rew and rec["rollout/ep_len_mean"] == length
        assert model.records[-1]["train/n_updates"] == 9 and model.records[-1]["time/iterations"] == 3
    # save / load: 4 iterations in one run == 2, save, load into fresh objects, 2 more (schedules and target_kl on)
    sched = dict(learning_rate=lambda p: 1e-3 * p, clip_range=lambda p: 0.1 + 0.2 * p, target_kl=0.05)
    per = B * n_steps
    env, policy, kw = _driver(B, n_steps, **sched)
    with env:
        whole = Ppo(env, policy, **kw).learn(4 * per)
        torch.cuda.synchronize()
        want, want_records = policy.packed.clone(), whole.records
    path = str(tmp_path / "ppo.pt")
    env, policy, kw = _driver(B, n_steps, **sched)
    with env:
        first = Ppo(env, policy, **kw).learn(4 * per, callback=lambda m, rec: m.iterations < 2)
        assert first.iterations == 2
        first.save(path)
    ends = []
    for _ in range(2):
        env, policy, kw = _driver(B, n_steps, **sched)
        with env:
            resumed = Ppo.load(path, env, policy, **kw)
            assert resumed.iterations == 2 and resumed.num_timesteps == 2 * per
            resumed.learn(2 * per, reset_num_timesteps=False)
            torch.cuda.synchronize()
            ends.append((policy.packed.clone(), resumed.records))
    assert torch.equal(ends[0][0], ends[1][0]) and ends[0][1] == ends[1][1], "two loads of the same file continue identically"
    print("resumed records:", ends[0][1][-1], "whole run:", want_records[-1])
    assert torch.equal(ends[0][0], want), "2 + save + load + 2 iterations equal 4 iterations, bit for bit"
    for a, b in zip(ends[0][1], want_records[2:]):
        assert a.keys() == b.keys()
        for key in a:
            assert a[key] == b[key] or (a[key] != a[key] and b[key] != b[key]), key


def test_learn_example_runs():
    env = dict(os.environ, EXAMPLE_STEPS="16")
    result = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_learn.py")], capture_output=True, text=True, timeout=600, env=env,
                            cwd=os.path.join(ROOT, "examples"))
    assert result.returncode == 0, result.stderr[-3000:]
    lines = [ln for ln in result.stdout.splitlines() if ln.startswith("iteration")]
    assert len(lines) >= 2 and all("train/loss" in ln for ln in lines), result.stdout
