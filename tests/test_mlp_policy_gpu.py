"""The MLP actor-critic launch (upkie_amd.policies.MlpActorCritic) on the MI355X: outputs against the fp64 twins of
tests/mlp_reference.py and the torch modules, sampling, buffer outputs, hipGraph replay, a closed loop, the example."""

import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import mlp_reference as R
from tests.mlp_shapes import CASES, DEV
from tests.mlp_shapes import policy as _policy
from tests.mlp_shapes import sources_of as _src
from tests.mlp_shapes import tower as _tower
from tests.training_rig import reset_pendulum
from upkie_amd.graphs import GraphedLoop
from upkie_amd.policies import MlpActorCritic, MlpPolicy
from upkie_amd.rollout import RolloutBuffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}" for c in CASES])
def test_deterministic_outputs_against_fp64_and_torch(case):
    N, D, widths, A, act = case
    pol, actor, critic, log_std = _policy(D, widths, A, act)
    obs = torch.randn(N, D, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    mean = torch.empty(N, A, device=DEV)
    env_action, action, value, log_prob = pol.act(obs, deterministic=True, out={"mean": mean})
    torch.cuda.synchronize()
    _, m64, v64 = R.forward(pol.shape, _src(pol), obs.double().cpu().numpy())
    assert np.abs(mean.double().cpu().numpy() - m64).max() <= 1e-5
    assert np.abs(value.double().cpu().numpy() - v64).max() <= 1e-5
    with torch.no_grad():
        assert (mean - actor(obs)).abs().max().item() <= 2e-5
        assert (value - critic(obs)[:, 0]).abs().max().item() <= 2e-5
    assert torch.equal(action, mean)
    assert torch.equal(env_action, mean.clamp(-1.0, 1.0))
    lp = R.log_prob(m64, m64, log_std.double().cpu().numpy())
    assert np.abs(log_prob.double().cpu().numpy() - lp).max() <= 1e-4
    assert int(pol.calls.abs().sum()) == 0, "deterministic calls do not advance the counters"
    v_only = pol.value(obs)
    assert torch.equal(v_only, value)


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=["6-relu", "30-tanh"])
def test_observation_normalisation(case):
    N, D, widths, A, act = case
    pol, actor, critic, _ = _policy(D, widths, A, act, normalize=True)
    obs = 2.0 * torch.randn(N, D, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    norm = torch.empty(N, D, device=DEV)
    mean = torch.empty(N, A, device=DEV)
    _, _, value, _ = pol.act(obs, deterministic=True, out={"norm_obs": norm, "mean": mean})
    torch.cuda.synchronize()
    x64, m64, v64 = R.forward(pol.shape, _src(pol), obs.double().cpu().numpy())
    assert np.abs(norm.double().cpu().numpy() - x64).max() <= 1e-6
    assert np.abs(mean.double().cpu().numpy() - m64).max() <= 1e-5
    assert np.abs(value.double().cpu().numpy() - v64).max() <= 1e-5
    with torch.no_grad():
        assert (mean - actor(norm)).abs().max().item() <= 2e-5


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[4]], ids=["4-1", "30-36", "5-3"])
def test_sampling(case):
    N, D, widths, A, act = case
    log_std = torch.linspace(-1.0, 0.5, A, device=DEV)
    pol, _, _, _ = _policy(D, widths, A, act, seed=3, log_std=log_std, low=-0.7, high=0.4)
    obs = torch.randn(N, D, device=DEV, generator=torch.Generator(DEV).manual_seed(7))
    mean = torch.empty(N, A, device=DEV)
    draws = []
    for call in range(2):
        env_action, action, value, log_prob = pol.act(obs, out={"mean": mean})
        draws.append([t.clone() for t in (env_action, action, log_prob, mean)])
    torch.cuda.synchronize()
    assert torch.equal(pol.calls, torch.full((N,), 2, dtype=torch.int32, device=DEV))
    sigma = torch.exp(log_std)
    n_check = min(N, 64)
    for call, (env_action, action, log_prob, m) in enumerate(draws):
        z = ((action - m) / sigma).double().cpu().numpy()
        twin = R.philox_normals(n_check, A, call, pol.seed)
        assert np.all(np.abs(z[:n_check] - twin) <= 1e-6 + 2e-7 * np.abs(twin)), np.abs(z[:n_check] - twin).max()
        want = torch.distributions.Normal(m.double(), sigma.double()).log_prob(action.double()).sum(-1)
        assert (log_prob.double() - want).abs().max().item() <= 1e-4
        assert torch.equal(env_action, torch.minimum(torch.maximum(action, pol.action_low), pol.action_high))
    assert not torch.equal(draws[0][1], draws[1][1]), "two calls draw different z"
    pol.reseed(pol.seed)
    again = pol.act(obs)
    assert torch.equal(again[1], draws[0][1]), "reseed reproduces the draws bit for bit"
    before = pol.calls.clone()
    pol.act(obs, deterministic=True)
    assert torch.equal(pol.calls, before)


def test_sb3_state_dict_builds_the_network_from_modules():
    """from_sb3_state_dict (Box-like and (low, high) action spaces, with and without a critic) packs exactly what
    from_modules packs for the same modules; unpack() reads every source back bit for bit."""
    torch.manual_seed(8)
    policy_net = nn.Sequential(nn.Linear(6, 64), nn.ReLU(), nn.Linear(64, 32), nn.ReLU()).to(DEV)
    value_net = nn.Sequential(nn.Linear(6, 48), nn.ReLU()).to(DEV)
    action_net, value_head = nn.Linear(32, 3).to(DEV), nn.Linear(48, 1).to(DEV)
    log_std = torch.tensor([-0.3, 0.1, -1.0], device=DEV)
    sd = {"log_std": log_std.cpu()}
    for prefix, mod in (("mlp_extractor.policy_net.", policy_net), ("mlp_extractor.value_net.", value_net), ("action_net.", action_net),
                        ("value_net.", value_head)):
        sd.update({prefix + k: v.cpu() for k, v in mod.state_dict().items()})
    low, high = np.array([-1.0, -0.5, -2.0], dtype=np.float32), np.array([1.0, 0.5, 2.0], dtype=np.float32)

    class Box:
        pass

    box = Box()
    box.low, box.high = low, high
    kw = dict(obs_mean=np.linspace(-1, 1, 6), obs_var=np.linspace(0.5, 2, 6), clip_obs=5.0, seed=4)
    want = MlpActorCritic.from_modules(nn.Sequential(*policy_net, action_net), nn.Sequential(*value_net, value_head), log_std, low, high, **kw)
    for space in (box, (low, high)):
        got = MlpActorCritic.from_sb3_state_dict(sd, "relu", space, device=DEV, **kw)
        assert torch.equal(got.packed, want.packed) and got.seed == want.seed
    for back, src in zip(want.unpack(), want.sources()):
        assert torch.equal(back, src.detach().reshape(-1).float())
    actor_only = {k: v for k, v in sd.items() if not k.startswith(("mlp_extractor.value_net", "value_net"))}
    got = MlpActorCritic.from_sb3_state_dict(actor_only, "relu", (low, high), device=DEV)
    ref = MlpActorCritic.from_modules(nn.Sequential(*policy_net, action_net), None, log_std, low, high)
    assert got.shape.critic_layers == 0 and torch.equal(got.packed, ref.packed)
    obs = torch.randn(100, 6, device=DEV)
    e, a, v, lp = got.act(obs, deterministic=True)
    assert v is None
    with pytest.raises(Exception, match="no critic"):
        got.value(obs)
    with pytest.raises(ValueError, match="serves batches of 100"):
        got.act(obs[:50])


def test_normal_moments():
    pol, _, _, _ = _policy(4, [16], 64, "tanh", log_std=torch.zeros(64, device=DEV), low=-1e30, high=1e30)
    obs = torch.randn(4096, 4, device=DEV)
    mean = torch.empty(4096, 64, device=DEV)
    _, action, _, _ = pol.act(obs, out={"mean": mean})
    z = (action - mean).double().reshape(-1)
    n = z.numel()
    assert abs(z.mean().item()) < 5 / math.sqrt(n)
    assert abs(z.var().item() - 1.0) < 5 * math.sqrt(2.0 / n)
    assert abs(((z - z.mean()) ** 3).mean().item()) < 5 * math.sqrt(15.0 / n)
    assert abs(((z - z.mean()) ** 4).mean().item() - 3.0) < 5 * math.sqrt(96.0 / n)


def test_buffer_outputs_and_no_allocation():
    N, T = 1000, 4
    pol, _, _, _ = _policy(6, [64, 64], 2, "relu")
    buf = RolloutBuffer(T, N, obs_shape=(6,), action_shape=(2,), device=DEV)
    obs = torch.randn(N, 6, device=DEV)
    env_action = torch.empty(N, 2, device=DEV)
    reward, start = torch.zeros(N, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV)
    pol.act(obs)  # (persistent buffers allocated)
    pol.reseed()
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated(DEV)
    for t in range(T):
        out = pol.act(obs, out={"action": buf.actions[t], "value": buf.values[t], "log_prob": buf.log_probs[t], "norm_obs": buf.observations[t],
                                "env_action": env_action})
        assert [o.data_ptr() for o in out] == [env_action.data_ptr(), buf.actions[t].data_ptr(), buf.values[t].data_ptr(), buf.log_probs[t].data_ptr()]
        buf.add_policy_step(None, reward, start, out)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(DEV) == allocated, "act(out=...) allocates nothing"
    assert buf.full
    pol.reseed()
    for t in range(T):
        e, a, v, lp = pol.act(obs)
        assert torch.equal(buf.actions[t], a) and torch.equal(buf.values[t], v) and torch.equal(buf.log_probs[t], lp)
        assert torch.equal(buf.observations[t], obs)


def test_graph_replay_is_bit_equal_to_the_eager_loop():
    """{policy -> env.step -> buffer slot} x 50, recorded as one hipGraph (GraphedLoop, unroll=50) and replayed, against
    the same 50 steps run eagerly from the same state and seed."""
    N, T = 4096, 50
    results = []
    for graphed in (False, True):
        pol, _, _, _ = _policy(4, [64, 64], 1, "tanh", seed=9, low=-0.9, high=0.9)
        with reset_pendulum(N) as env:
            obs = env.observation
            buf = RolloutBuffer(T, N, obs_shape=(4,), action_shape=(1,), device=env.device)
            env_action = torch.empty(N, 1, device=env.device)
            slot = {"t": 0}

            def body():
                t = slot["t"]
                pol.act(obs, out={"action": buf.actions[t], "value": buf.values[t], "log_prob": buf.log_probs[t], "norm_obs": buf.observations[t],
                                  "env_action": env_action})
                _, reward, terminated, truncated, _ = env.step(env_action)
                buf.rewards[t].copy_(reward)
                slot["t"] = (t + 1) % T

            keep = list(env.state_tensors().values())  # (`obs` among them)
            saved = [x.clone() for x in keep]
            if graphed:
                loop = GraphedLoop(body, unroll=T, warmup=1)  # (warm-up and capture advance the state: restored below)
                for x, s in zip(keep, saved):
                    x.copy_(s)
                pol.reseed()
                loop.replay()
            else:
                slot["t"] = 1  # (the slot order of the capture, which follows one warm-up step)
                for _ in range(T):
                    body()
            torch.cuda.synchronize()
            results.append([buf.actions.clone(), buf.values.clone(), buf.log_probs.clone(), buf.observations.clone(), buf.rewards.clone()])
    for eager, graph in zip(*results):
        assert torch.equal(eager, graph)


def test_closed_loop_against_torch_modules_per_step():
    N, T = 4096, 400
    torch.manual_seed(4)
    actor = _tower(4, [64, 64], 1, "tanh").to(DEV)
    policy = MlpPolicy.from_modules(actor, torch.tensor([-1.0]), torch.tensor([1.0]))
    worst = 0.0
    with reset_pendulum(N, seed=1) as env, torch.no_grad():
        obs = env.observation
        for _ in range(T):
            action = policy(obs)
            worst = max(worst, (action - actor(obs).clamp(-1.0, 1.0)).abs().max().item())
            obs, *_ = env.step(action)
    assert worst <= 2e-5, worst


def test_example_runs():
    env = dict(os.environ, EXAMPLE_STEPS="8")
    result = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_mlp_rollout.py")], capture_output=True, text=True, timeout=600, env=env,
                            cwd=os.path.join(ROOT, "examples"))
    assert result.returncode == 0, result.stderr[-3000:]
    assert "ppo_mlp_rollout:" in result.stdout
