"""The PPO update (upkie_amd.ppo.PpoTrainer, csrc/ppo.hpp) on the MI355X: gradient, clip and Adam against the fp64 twin
of tests/ppo_reference.py and against torch fp32, determinism and graph replay, the fixed words, the write-back, the
example."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import ppo_reference as R
from tests.mlp_shapes import CASES, IDS, WIDEST, T
from tests.mlp_shapes import restore_trainer as _restore
from tests.mlp_shapes import tower as _tower
from tests.mlp_shapes import trainer_case as _setup
from tests.mlp_shapes import trainer_state as _state
from upkie_amd.exceptions import UpkieRuntimeError
from upkie_amd.normalize import RunningNormalizer
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import PpoTrainer, trainable_offset
from upkie_amd.rollout import RolloutBuffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BETA1_F32 = np.float32(1.0) - np.float32(0.9)


def _np(t):
    return t.detach().double().cpu().numpy()


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.mark.parametrize("case", CASES + [WIDEST], ids=IDS + ["widest"])
def test_one_minibatch_gradient_against_the_fp64_twin(case):
    pol, _, _, _, buf = _setup(case, normalize=case[1] == 6)
    tr = PpoTrainer(pol, n_epochs=1, batch_size=T * case[0], max_grad_norm=1e9, ent_coef=0.01, clip_range_vf=0.2, seed=3)
    src0 = [_np(s) for s in pol.sources()]
    stats = tr.train(buf)
    torch.cuda.synchronize()
    idx = tr.perm[0].long().cpu().numpy()
    # the twin on the weights before the step
    shape = pol.shape
    x = _np(buf.observations).reshape(-1, case[1])[idx]
    flat = lambda t: _np(t).reshape(-1)[idx]  # noqa: E731
    ref_stats, ref_grads, ratio = R.minibatch(shape, src0, x, _np(buf.actions).reshape(-1, case[3])[idx], flat(buf.values), flat(buf.log_probs),
                                              flat(buf.advantages), flat(buf.returns), ent_coef=0.01, clip_range_vf=0.2, max_grad_norm=1e9)
    for bound in (0.8, 1.2):
        assert not (np.abs(ratio - bound) < 1e-4).any(), "no sample's ratio within 1e-4 of a clip bound"
    m = tr.state_dict()["m"]
    for k, (mm, g) in enumerate(zip(m, ref_grads)):
        got = _np(mm).reshape(g.shape) / float(BETA1_F32)
        assert _rel(got, g) <= 1e-5, (k, _rel(got, g))
    s = stats.double().cpu().numpy()[0, 0]
    np.testing.assert_allclose(s[[0, 1, 2, 3, 6]], ref_stats[[0, 1, 2, 3, 6]], rtol=1e-4, atol=1e-6)
    assert abs(s[4] - ref_stats[4]) <= 1e-5 and abs(s[5] - ref_stats[5]) <= 1.0 / (T * case[0])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_full_update_against_the_fp64_twin(case):
    pol, _, _, _, buf = _setup(case, seed=1, first=True)
    lr = 1e-3
    tr = PpoTrainer(pol, lr=lr, n_epochs=1, batch_size=T * case[0], seed=5)
    src0 = [_np(s) for s in pol.sources()]
    packed0 = pol.packed.clone()
    stats = tr.train(buf)
    torch.cuda.synchronize()
    idx = tr.perm[0].long().cpu().numpy()
    flat = lambda t: _np(t).reshape(-1)[idx]  # noqa: E731
    ref_stats, grads, ratio = R.minibatch(pol.shape, src0, _np(buf.observations).reshape(-1, case[1])[idx],
                                          _np(buf.actions).reshape(-1, case[3])[idx], flat(buf.values), flat(buf.log_probs), flat(buf.advantages),
                                          flat(buf.returns))
    assert np.all(np.abs(ratio - 1.0) < 1e-4), "first minibatch: every ratio ties at 1"
    params0 = R.trainable(pol.shape, src0)
    zeros = [0 * g for g in grads]
    params, m, v, t = R.adam_step(params0, grads, zeros, zeros, 0, 0.5, lr)
    sd = tr.state_dict()
    assert sd["t"] == 1 and sd["lr"] == pytest.approx(lr)
    after = [_np(p) for p in pol.sources()[4:]]
    coef = min(1.0, 0.5 / (ref_stats[6] + 1e-6))
    for k, (p1, p0, pr, g) in enumerate(zip(after, params0, params, grads)):
        p1 = p1.reshape(pr.shape)
        # a gradient error delta (|delta| <= 1e-5 ||g|| of the tensor, relative) moves Adam's first step by about lr delta / (|g| + eps)
        delta = 1e-5 * np.linalg.norm(g) * coef + 1e-6 * np.abs(g) * coef
        bound = lr * delta / (np.abs(g) * coef + 1e-5) + 2e-7 * np.abs(p0) + 1e-9
        assert np.all(np.abs((p1 - p0) - (pr - p0)) <= bound), (k, np.max(np.abs((p1 - p0) - (pr - p0)) / bound))
    for got, want in ((sd["m"], m), (sd["v"], v)):
        for a, b in zip(got, want):
            assert _rel(_np(a).reshape(b.shape), b) <= 1e-4
    s = stats.double().cpu().numpy()[0, 0]
    np.testing.assert_allclose(s[[0, 1, 2, 3, 6]], ref_stats[[0, 1, 2, 3, 6]], rtol=1e-4, atol=1e-6)
    assert abs(s[4]) <= 1e-6 and s[5] == 0.0, "ratio 1: no KL, nothing clipped"
    fixed = trainable_offset(pol.shape)
    assert torch.equal(pol.packed[:fixed], packed0[:fixed]), "the fixed words are never written"


def _torch_epoch(actor, critic, log_std, buf, perm, batch, lr):
    """One SB3 epoch of minibatches in torch fp32 on the GPU (autograd, clip_grad_norm_, Adam(eps=1e-5))."""
    params = [log_std] + [p for seq in (actor, critic) for m in seq if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]
    opt = torch.optim.Adam(params, lr=lr, eps=1e-5)
    total = perm.numel()
    flat = {"obs": buf.observations.reshape(total, -1), "act": buf.actions.reshape(total, -1), "v": buf.values.reshape(total),
            "lp": buf.log_probs.reshape(total), "adv": buf.advantages.reshape(total), "ret": buf.returns.reshape(total)}
    stats = []
    for start in range(0, total, batch):
        i = perm[start:start + batch].long()
        adv = flat["adv"][i]
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        mean = actor(flat["obs"][i])
        dist = torch.distributions.Normal(mean, torch.ones_like(mean) * log_std.exp())
        ratio = torch.exp(dist.log_prob(flat["act"][i]).sum(1) - flat["lp"][i])
        pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 0.8, 1.2)).mean()
        vl = nn.functional.mse_loss(flat["ret"][i], critic(flat["obs"][i]).flatten())
        loss = pl + 0.5 * vl
        opt.zero_grad()
        loss.backward()
        norm = nn.utils.clip_grad_norm_(params, 0.5)
        opt.step()
        stats.append([pl.item(), vl.item(), loss.item(), float(norm)])
    return params, np.array(stats)


@pytest.mark.parametrize("case", [CASES[0], CASES[4]], ids=[IDS[0], IDS[4]])
def test_one_epoch_of_four_minibatches_against_torch_fp32(case):
    pol, actor, critic, log_std, buf = _setup(case, seed=2)
    total = T * case[0]
    batch = (total + 3) // 4
    lr = 3e-4
    ref_actor, ref_critic = _tower(case[1], case[2], case[3], case[4]).to(DEV), _tower(case[1], case[2], 1, case[4]).to(DEV)
    ref_actor.load_state_dict(actor.state_dict())
    ref_critic.load_state_dict(critic.state_dict())
    ref_log_std = nn.Parameter(log_std.detach().clone())
    before = [p.detach().clone() for p in [ref_log_std] + [p for s in (ref_actor, ref_critic) for m in s if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]]
    tr = PpoTrainer(pol, lr=lr, n_epochs=1, batch_size=batch, seed=11)
    stats = tr.train(buf)
    params, ref_stats = _torch_epoch(ref_actor, ref_critic, ref_log_std, buf, tr.perm[0], batch, lr)
    torch.cuda.synchronize()
    # Adam's step is lr * m / (sqrt(v) + eps) per word: fp32 rounding of a gradient word near zero (relative to the
    # rounding of the sums behind it) may turn its step by up to ~lr per minibatch; such words are few, so the deltas
    # agree as tensors to 2 % while the losses, computed before each step, agree to fp32 summation order (1e-4).
    ours = [log_std] + [p for s in (actor, critic) for m in s if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]
    for k, (a, b, p0) in enumerate(zip(ours, params, before)):
        da, db = _np(a) - _np(p0), _np(b) - _np(p0)
        assert _rel(da, db) <= 2e-2, (k, _rel(da, db))
        assert np.all(np.abs(da - db) <= 4 * 4 * lr + 1e-6)
    s = stats.double().cpu().numpy()[0]
    np.testing.assert_allclose(s[:, [0, 1, 3, 6]], ref_stats, rtol=2e-3, atol=2e-5)


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[4]], ids=[IDS[0], IDS[2], IDS[4]])
def test_deterministic_and_graph_replay_bit_identical(case):
    pol, _, _, _, buf = _setup(case, seed=3)
    tr = PpoTrainer(pol, n_epochs=2, batch_size=(T * case[0] + 2) // 3, seed=1, ent_coef=0.003)
    tr.prepare(buf)
    s0 = _state(pol, tr)
    runs = []
    for _ in range(2):
        _restore(pol, tr, s0)
        stats = tr.update(buf, sync=False).clone()
        torch.cuda.synchronize()
        runs.append(_state(pol, tr) + [stats])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], s0[0]), "training moved the weights"
    _restore(pol, tr, s0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr.update(buf, sync=False)
    _restore(pol, tr, s0)  # (capture records, it does not run)
    tr.stats.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(_state(pol, tr) + [tr.stats], runs[0]):
        assert torch.equal(a, b)
    t_before = float(tr.scalars[1])
    tr.set_lr(1e-4)
    graph.replay()  # the next iteration: t advances, the new lr is read
    torch.cuda.synchronize()
    assert float(tr.scalars[1]) == t_before + tr.n_epochs * tr.n_minibatches and float(tr.scalars[0]) == 1e-4


def test_normalizer_words_are_untouched_and_raw_observations_refused():
    N, D, widths, A, act = CASES[0]
    torch.manual_seed(0)
    actor, critic = _tower(D, widths, A, act).to(DEV), _tower(D, widths, 1, act).to(DEV)
    log_std = nn.Parameter(torch.zeros(A, device=DEV))
    pol = MlpActorCritic.from_modules(actor, critic, log_std, [-1.0], [1.0], seed=0)
    norm = RunningNormalizer(N, D, device=DEV)
    norm.attach(pol)
    buf = RolloutBuffer(T, N, obs_shape=(D,), action_shape=(A,), device=DEV)
    gen = torch.Generator(DEV).manual_seed(3)
    obs = torch.randn(N, D, device=DEV, generator=gen) * 2 + 0.5
    norm.reset(obs)
    for t in range(T):
        pol.act(obs, out={"norm_obs": buf.observations[t], "action": buf.actions[t], "value": buf.values[t], "log_prob": buf.log_probs[t]})
        obs = torch.randn(N, D, device=DEV, generator=gen) * 2 + 0.5
        norm.step(obs, torch.randn(N, device=DEV, generator=gen), out={"reward": buf.rewards[t]})
    buf.pos, buf.full = T, True
    buf.compute_returns_and_advantage(last_values=pol.value(obs), dones=torch.zeros(N, dtype=torch.uint8, device=DEV))
    fixed = trainable_offset(pol.shape)
    before = pol.packed[:fixed].clone()
    with pytest.raises(UpkieRuntimeError, match="RunningNormalizer"):
        PpoTrainer(pol, n_epochs=1, batch_size=N).train(buf)
    tr = PpoTrainer(pol, n_epochs=3, batch_size=N // 2, obs_normalized=True)
    tr.train(buf)
    torch.cuda.synchronize()
    assert torch.equal(pol.packed[:fixed], before), "obs_mean / obs_std / action bounds bit-unchanged"
    assert not torch.equal(pol.packed[fixed:], pol.packed[fixed:] * 0)


def test_write_back_act_equals_a_fresh_policy_and_update_from_is_a_no_op():
    pol, actor, critic, log_std, buf = _setup(CASES[4], seed=4, normalize=True)
    tr = PpoTrainer(pol, n_epochs=2, batch_size=500, lr=1e-3)
    before = pol.packed.clone()
    tr.train(buf)
    torch.cuda.synchronize()
    assert not torch.equal(before, pol.packed)
    trained = pol.packed.clone()
    pol.update_from()
    assert torch.equal(pol.packed, trained), "update_from() after train() is a bitwise no-op"
    N, D, widths, A, act = CASES[4]
    g = torch.Generator().manual_seed(5)  # (_setup's statistics)
    fresh = MlpActorCritic.from_modules(actor, critic, log_std, torch.full((A,), -1.0), torch.full((A,), 1.0), seed=9,
                                        obs_mean=0.3 * torch.randn(D, generator=g), obs_var=torch.rand(D, generator=g) * 3 + 0.2, clip_obs=3.0)
    assert torch.equal(fresh.packed, trained)
    obs = torch.randn(N, D, device=DEV, generator=torch.Generator(DEV).manual_seed(8))
    a = [t.clone() for t in pol.act(obs, deterministic=True)]
    b = fresh.act(obs, deterministic=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_example_runs():
    env = dict(os.environ, EXAMPLE_STEPS="16")
    result = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_mlp_train.py")], capture_output=True, text=True, timeout=600, env=env,
                            cwd=os.path.join(ROOT, "examples"))
    assert result.returncode == 0, result.stderr[-3000:]
    lines = [ln for ln in result.stdout.splitlines() if ln.startswith("iteration")]
    assert len(lines) >= 2 and all("nan" not in ln for ln in lines), result.stdout


@pytest.mark.parametrize("case", [CASES[0], CASES[4]], ids=[IDS[0], IDS[4]])
def test_captured_update_reads_each_iterations_fresh_advantages(case):
    """compute_returns_and_advantage allocates new advantages and returns every iteration; a captured update replayed
    after prepare(buffer) must train on the new ones: bit for bit the eager update on the same data."""
    pol, _, _, _, buf = _setup(case, seed=6)
    N = case[0]
    gen = torch.Generator(DEV).manual_seed(17)

    def rollout_data():
        buf.rewards.copy_(torch.randn(T, N, device=DEV, generator=gen))
        buf.compute_returns_and_advantage(last_values=torch.randn(N, device=DEV, generator=gen),
                                          dones=torch.zeros(N, dtype=torch.uint8, device=DEV))

    rollout_data()
    tr = PpoTrainer(pol, n_epochs=2, batch_size=(T * N + 1) // 2, seed=2)
    tr.prepare(buf)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr.update(buf, sync=False)
    previous = None
    for _ in range(3):
        rollout_data()  # new advantage / return tensors; the old ones are freed
        junk = [torch.full((T, N), 1e3, device=DEV) for _ in range(4)]  # (would take over a freed block a stale launch reads)
        tr.prepare(buf)
        assert previous is None or not torch.equal(tr.advantages, previous)
        previous = tr.advantages.clone()
        s0 = _state(pol, tr)
        graph.replay()
        torch.cuda.synchronize()
        replayed = _state(pol, tr) + [tr.stats.clone()]
        _restore(pol, tr, s0)
        tr.update(buf, sync=False)
        torch.cuda.synchronize()
        for a, b in zip(_state(pol, tr) + [tr.stats], replayed):
            assert torch.equal(a, b)
        del junk
    other = RolloutBuffer(T, N, obs_shape=(case[1],), action_shape=(case[3],), device=DEV)
    other.advantages, other.returns, other.pos, other.full = buf.advantages, buf.returns, T, True
    with pytest.raises(ValueError, match="one rollout buffer"):
        tr.prepare(other)
