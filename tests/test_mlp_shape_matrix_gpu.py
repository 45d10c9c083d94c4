"""Every instantiation and block geometry of the MLP kernels on the MI355X, against the fp64 twins: the policy launch,
the time-limit bootstrap and the PPO gradient launch on every row of tests/mlp_shapes.py's MATRIX (all ten (width class,
activation) pairs, gradient blocks of 1 to 4 waves, grids below and above the cap, asymmetric towers, observations past
the first load chunk, partly filled action tiles). tests/test_mlp_shape_matrix.py proves on the host that the table
covers this and that a dropped unit of any layer would exceed the bounds applied here.

Each test prints a line `matrix <family> <id> <figure>=<value> ...` with the kernel's and torch fp32's distance to the
fp64 twin before it asserts: profiles/mlp_shape_matrix.txt is that output."""

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import mlp_reference as R
from tests import mlp_shapes as S
from tests import ppo_reference as PR
from tests.test_time_limits_gpu import _check_bootstrap
from upkie_amd.ppo import PpoTrainer
from upkie_amd.rollout import RolloutBuffer

pytestmark = pytest.mark.gpu
DEV = S.DEV
T = S.T
BETA1_F32 = np.float32(1.0) - np.float32(0.9)


def _geometry(row):
    shape = S.shape_of(row)
    return S.width_class(shape), PR.plan(shape)


def _param(index, row):
    W, plan = _geometry(row)
    return pytest.param(index, row, id=f"W{W}-{row.activation}-nw{plan['nw']}-{S.row_id(row)}")


ROWS = [_param(i, r) for i, r in enumerate(S.MATRIX)]


def _report(family, row, **figures):
    print(f"\nmatrix {family} {S.row_id(row)} " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))


def _np(t):
    return t.detach().double().cpu().numpy()


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _policy(index, row, **kw):
    return S.policy(row.obs_dim, row.actor, row.act_dim, row.activation, seed=row.seed, normalize=S.row_normalize(index), critic_widths=row.critic, **kw)


def _host_sources_are_the_device_sources(index, row, pol):
    """The row as tests/test_mlp_shape_matrix.py sees it (host modules) is the policy on the device, word for word."""
    host = S.row_sources(row, *S.row_modules(row), S.row_normalize(index))
    for k, (a, b) in enumerate(zip(host, S.sources_of(pol))):
        if k not in (2, 3, 4):  # (action bounds and log_std are the test's own)
            assert np.array_equal(np.asarray(a).reshape(-1), b.reshape(-1)), k


def _normalised(pol, obs):
    """The policy's observation normalisation as torch fp32 ops."""
    if not pol.shape.normalize:
        return obs
    mean, std = pol.sources()[0], pol.sources()[1]
    return ((obs - mean) / std).clamp(-pol.clip_obs, pol.clip_obs)


# ---------------------------------------------------------------- policy launch
@pytest.mark.parametrize("index,row", ROWS)
def test_policy_against_the_fp64_twin(index, row):
    N, D, A = row.N, row.obs_dim, row.act_dim
    bound = S.bounds(row)
    normalize = S.row_normalize(index)
    log_std = torch.linspace(-1.0, 0.5, A, device=DEV)
    pol, actor, critic, _ = _policy(index, row, log_std=log_std, low=-0.7, high=0.4)
    _host_sources_are_the_device_sources(index, row, pol)
    obs = S.row_observations(row, scale=2.0 if normalize else 1.0).to(DEV)
    mean, norm = torch.empty(N, A, device=DEV), torch.empty(N, D, device=DEV)
    env_action, action, value, log_prob = pol.act(obs, deterministic=True, out={"mean": mean, "norm_obs": norm})
    torch.cuda.synchronize()
    x64, m64, v64 = R.forward(pol.shape, S.sources_of(pol), _np(obs))
    with torch.no_grad():
        x32 = _normalised(pol, obs)
        torch_mean, torch_value = np.abs(_np(actor(x32)) - m64).max(), np.abs(_np(critic(x32)[:, 0]) - v64).max()
    err_mean, err_value, err_norm = np.abs(_np(mean) - m64).max(), np.abs(_np(value) - v64).max(), np.abs(_np(norm) - x64).max()
    lp = R.log_prob(m64, m64, _np(log_std))
    err_lp = np.abs(_np(log_prob) - lp).max()
    _report("policy", row, mean=float(err_mean), torch_mean=float(torch_mean), bound_mean=bound["mean"], value=float(err_value),
            torch_value=float(torch_value), bound_value=bound["value"], norm_obs=float(err_norm), log_prob=float(err_lp))
    assert err_norm <= bound["norm_obs"]
    assert err_mean <= bound["mean"]
    assert err_value <= bound["value"]
    assert err_lp <= bound["log_prob"]
    assert torch.equal(action, mean)
    assert torch.equal(env_action, mean.clamp(-0.7, 0.4))
    assert int(pol.calls.abs().sum()) == 0, "deterministic calls do not advance the counters"
    # the value-only call: the same bits as the fused call (into a tensor of its own: `value` is the persistent buffer)
    fused = value.clone()
    v_only = pol.value(obs, out=torch.full((N,), float("nan"), device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(v_only.view(torch.int32), fused.view(torch.int32))

    # one sampling call: z of every action column, on the first tile and the last two (the partial one included)
    env_action, action, value, log_prob = pol.act(obs, out={"mean": mean})
    torch.cuda.synchronize()
    assert torch.equal(pol.calls, torch.ones(N, dtype=torch.int32, device=DEV)), "the counters advance by one"
    assert torch.equal(value.view(torch.int32), fused.view(torch.int32))
    sigma = torch.exp(log_std)
    z = _np((action - mean) / sigma)
    envs = sorted(set(range(min(N, 16))) | set(range(max(0, 16 * ((N - 1) // 16) - 16), N)))
    twin = np.array([[R.philox_normal(e, 0, a, pol.seed) for a in range(A)] for e in envs])
    assert np.all(np.abs(z[envs] - twin) <= 1e-6 + 2e-7 * np.abs(twin)), np.abs(z[envs] - twin).max()
    want = torch.distributions.Normal(mean.double(), sigma.double()).log_prob(action.double()).sum(-1)
    assert (log_prob.double() - want).abs().max().item() <= bound["log_prob"]
    assert torch.equal(env_action, torch.minimum(torch.maximum(action, pol.action_low), pol.action_high))
    assert np.abs(_np(mean) - m64).max() <= bound["mean"]


# ---------------------------------------------------------------- time-limit bootstrap
@pytest.mark.parametrize("index,row", ROWS)
def test_bootstrap_is_the_policys_value_bit_for_bit(index, row):
    """tests/test_time_limits_gpu.py's check (bit-equality with `pol.value`, every mask kind, the fp64 twin): it holds
    only if the bootstrap and the policy kernel run the critic identically in this instantiation."""
    pol, _, _, _ = _policy(index, row)
    _check_bootstrap(pol, row.N, row.obs_dim, seed=11)


# ---------------------------------------------------------------- PPO gradient launch
def _torch_gradient(pol, actor, critic, log_std, buf, total):
    """SB3's minibatch loss over the whole buffer in torch fp32 on the device, its gradient by autograd: log_std, then
    (weight, bias) per layer of the actor and of the critic."""
    params = [log_std] + [p for seq in (actor, critic) for m in seq if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]
    x = _normalised(pol, buf.observations.reshape(total, -1))
    adv = buf.advantages.reshape(total)
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    old_v, ret = buf.values.reshape(total), buf.returns.reshape(total)
    mean = actor(x)
    dist = torch.distributions.Normal(mean, torch.ones_like(mean) * log_std.exp())
    ratio = torch.exp(dist.log_prob(buf.actions.reshape(total, -1)).sum(1) - buf.log_probs.reshape(total))
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 0.8, 1.2)).mean()
    v = critic(x).flatten()
    value_loss = nn.functional.mse_loss(ret, old_v + torch.clamp(v - old_v, -0.2, 0.2))
    loss = policy_loss + 0.01 * (-dist.entropy().sum(1).mean()) + 0.5 * value_loss
    grads = torch.autograd.grad(loss, params)
    return [_np(g) for g in grads]


@pytest.mark.parametrize("index,row", ROWS)
def test_gradient_against_the_fp64_twin(index, row):
    """tests/test_ppo_gpu.py's one-minibatch gradient check on every row: T = 2, one minibatch of all samples, no
    gradient clipping; on the rows whose blocks hold 2 or 3 waves or take more than one chunk, also the bit-identical
    repeat from the same state."""
    N, D, A = row.N, row.obs_dim, row.act_dim
    total = T * N
    bound = S.bounds(row)
    W, plan = _geometry(row)
    log_std = nn.Parameter(torch.full((A,), -0.5, device=DEV))
    pol, actor, critic, _ = _policy(index, row, log_std=log_std)
    _host_sources_are_the_device_sources(index, row, pol)
    src0 = S.sources_of(pol)
    data = S.row_rollout(row, pol.shape, src0)
    buf = RolloutBuffer(T, N, obs_shape=(D,), action_shape=(A,), device=DEV)
    for name in ("observations", "actions", "values", "log_probs"):
        getattr(buf, name).copy_(torch.as_tensor(data[name], device=DEV).reshape(getattr(buf, name).shape))
    buf.advantages = torch.as_tensor(data["advantages"], device=DEV)
    buf.returns = torch.as_tensor(data["returns"], device=DEV)
    buf.pos, buf.full = T, True
    torch_grads = _torch_gradient(pol, actor, critic, log_std, buf, total)

    tr = PpoTrainer(pol, n_epochs=1, batch_size=total, max_grad_norm=1e9, ent_coef=0.01, clip_range_vf=0.2, seed=3)
    tr.prepare(buf)
    state0 = [t.clone() for t in (pol.packed, tr.m, tr.v, tr.scalars)]
    stats = tr.update(buf)
    torch.cuda.synchronize()
    idx = tr.perm[0].long().cpu().numpy()
    flat = lambda k, *tail: data[k].astype(np.float64).reshape(total, *tail)[idx]  # noqa: E731
    ref_stats, ref_grads, ratio = PR.minibatch(pol.shape, src0, flat("observations", D), flat("actions", A), flat("values"), flat("log_probs"),
                                               flat("advantages"), flat("returns"), ent_coef=0.01, clip_range_vf=0.2, max_grad_norm=1e9)
    for edge in (0.8, 1.2):
        assert not (np.abs(ratio - edge) < 1e-4).any(), "no sample's ratio within 1e-4 of a clip bound"
    assert (ratio < 0.8).any() and (ratio > 1.2).any() or total < 8, "samples clipped on both sides"
    m = tr.state_dict()["m"]
    assert len(m) == len(ref_grads) == len(torch_grads)
    errors = [_rel(_np(mm).reshape(g.shape) / float(BETA1_F32), g) for mm, g in zip(m, ref_grads)]
    torch_errors = [_rel(tg.reshape(g.shape), g) for tg, g in zip(torch_grads, ref_grads)]
    worst = int(np.argmax(errors))
    _report("gradient", row, W=W, nw=plan["nw"], chunks=PR.chunks(plan, total), grid_cap=plan["grid_cap"], worst_tensor=worst,
            grad=float(errors[worst]), torch_grad=float(torch_errors[worst]), torch_grad_max=float(max(torch_errors)), bound_grad=bound["grad"])
    for k, e in enumerate(errors):
        assert e <= bound["grad"], (k, e, torch_errors[k])
    s = stats.double().cpu().numpy()[0, 0]
    np.testing.assert_allclose(s[[0, 1, 2, 3, 6]], ref_stats[[0, 1, 2, 3, 6]], rtol=1e-4, atol=1e-6)
    assert abs(s[4] - ref_stats[4]) <= 1e-5 and abs(s[5] - ref_stats[5]) <= 1.0 / total

    if plan["nw"] in (2, 3) or PR.chunks(plan, total) > plan["grid_cap"]:
        first = [t.clone() for t in (pol.packed, tr.m, tr.v, tr.scalars, stats)]
        for dst, src in zip((pol.packed, tr.m, tr.v, tr.scalars), state0):
            dst.copy_(src)
        again = tr.update(buf, sync=False)
        torch.cuda.synchronize()
        for a, b in zip((pol.packed, tr.m, tr.v, tr.scalars, again), first):
            assert torch.equal(a, b), "two updates from the same state give the same bits"
        assert not torch.equal(pol.packed, state0[0]), "the update moved the weights"
