"""PPO.learn's new pieces without a GPU: the fp64 twin of the whole update (tests/ppo_learn_reference.py) against a
torch-autograd transcription of Stable-Baselines3's ``PPO.train`` loop with ``target_kl``; the argument checks of the
control-block entry points through the built library; `PpoTrainer`'s schedule handling; `Ppo.learn`'s bookkeeping
against a fake trainer."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import mlp_reference as MR
from tests import ppo_learn_reference as L
from tests import ppo_reference as R
from tests.agent_step_doubles import filler, saved_parts, stage
from tests.test_ppo import _modules, _shape, _sources
from upkie_amd import abi, lib
from upkie_amd.exceptions import UpkieRuntimeError
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import Ppo, PpoTrainer


@pytest.fixture(scope="module")
def library():
    lib.build()
    return lib.load()


def _torch_sb3_train(actor, critic, log_std, data, perms, batch_size, c, target_kl):
    """SB3 PPO.train, literally, in float64: the epoch and minibatch loops, the loss and its gradient (autograd), the
    target_kl check before the step, clip_grad_norm_, Adam, _n_updates."""
    params = [log_std] + [p for seq in (actor, critic) for m in seq if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]
    opt = torch.optim.Adam(params, lr=c["lr"], eps=1e-5)
    n_updates, continue_training, stopped_at, kls = 0, True, None, []
    total = len(perms[0])
    for epoch in range(len(perms)):
        approx_kl_divs = []
        for j, start in enumerate(range(0, total, batch_size)):
            i = torch.as_tensor(np.asarray(perms[epoch][start:start + batch_size], dtype=np.int64))
            adv = data["advantages"][i]
            if c["normalize_advantage"] and len(adv) > 1:
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            mean = actor(data["obs"][i])
            dist = torch.distributions.Normal(mean, torch.ones_like(mean) * log_std.exp())
            log_prob = dist.log_prob(data["actions"][i]).sum(dim=1)
            entropy = dist.entropy().sum(dim=1)
            values = critic(data["obs"][i]).flatten()
            ratio = torch.exp(log_prob - data["old_log_prob"][i])
            policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - c["clip_range"], 1 + c["clip_range"])).mean()
            value_loss = torch.nn.functional.mse_loss(data["returns"][i], values)
            entropy_loss = -torch.mean(entropy)
            loss = policy_loss + c["ent_coef"] * entropy_loss + c["vf_coef"] * value_loss
            with torch.no_grad():
                log_ratio = log_prob - data["old_log_prob"][i]
                approx_kl_div = torch.mean((torch.exp(log_ratio) - 1) - log_ratio).cpu().numpy()
                approx_kl_divs.append(approx_kl_div)
                kls.append(float(approx_kl_div))
            if target_kl is not None and approx_kl_div > 1.5 * target_kl:
                continue_training = False
                stopped_at = (epoch, j)
                break
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, c["max_grad_norm"])
            opt.step()
        n_updates += 1
        if not continue_training:
            break
    state = [(opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy()) for p in params]
    return [p.detach().numpy().copy() for p in params], state, n_updates, stopped_at, kls


def _problem(seed=0, B=96, D=5, widths=(24, 16), A=2, act="tanh"):
    rng = np.random.default_rng(seed)
    actor, critic = _modules(D, list(widths), A, act, seed=seed)
    log_std = torch.tensor(rng.normal(-0.5, 0.2, size=A), requires_grad=True)
    mean, std = np.zeros(D), np.ones(D)
    shape = _shape(D, list(widths), A, act, normalize=False)
    src = _sources(actor, critic, log_std, D, A, mean, std)
    obs = rng.normal(0, 1.0, size=(B, D))
    with torch.no_grad():
        mu = actor(torch.as_tensor(obs)).numpy()
        v = critic(torch.as_tensor(obs)).numpy()[:, 0]
    actions = mu + np.exp(log_std.detach().numpy()) * rng.normal(size=(B, A))
    data = dict(obs=obs, actions=actions, old_values=v + rng.normal(0, 0.2, B), old_log_prob=MR.log_prob(actions, mu, log_std.detach().numpy()),
                advantages=rng.normal(0, 1.0, B), returns=v + rng.normal(0, 1.0, B))
    perms = [rng.permutation(B) for _ in range(4)]
    return shape, src, data, perms, actor, critic, log_std


def test_fp64_twin_is_torch_autograd_of_sb3s_train_loop_with_target_kl():
    shape, src, data, perms, actor, critic, log_std = _problem()
    over = dict(lr=1e-2, ent_coef=0.01)
    c = dict(R.DEFAULTS, **over)
    free = L.train(shape, src, data, perms, 24, target_kl=None, obs_normalized=True, **over)
    assert free["stopped_at"] is None and free["applied"] == 16 and free["n_updates"] == 4
    chosen = L.choose_target_kl(free["rows"][:, 4])
    assert chosen is not None, free["rows"][:, 4]
    target_kl, k = chosen
    assert 0 < k < 15
    twin = L.train(shape, src, data, perms, 24, target_kl=target_kl, obs_normalized=True, **over)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    want_params, want_state, want_updates, want_stop, want_kls = _torch_sb3_train(actor, critic, log_std, {k_: t(x) for k_, x in data.items()}, perms,
                                                                                 24, c, target_kl)
    assert twin["stopped_at"] == want_stop == divmod(k, 4)
    assert twin["n_updates"] == want_updates == k // 4 + 1 and twin["applied"] == k == twin["t"]
    np.testing.assert_allclose(twin["rows"][:, 4], want_kls, rtol=1e-9, atol=1e-15)
    for p, w, mm, vv, (wm, wv) in zip(twin["params"], want_params, twin["m"], twin["v"], want_state):
        np.testing.assert_allclose(p, w.reshape(p.shape), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(mm, wm.reshape(mm.shape), rtol=1e-12, atol=1e-18)
        np.testing.assert_allclose(vv, wv.reshape(vv.shape), rtol=1e-12, atol=1e-24)
    rec = twin["record"]
    assert rec["early_stopped_at"] == want_stop and rec["n_updates"] == want_updates
    assert rec["approx_kl"] == pytest.approx(np.mean(want_kls), rel=1e-9)
    assert rec["explained_variance"] == pytest.approx(1.0 - np.var(data["returns"] - data["old_values"]) / np.var(data["returns"]), rel=1e-12)
    assert math.isnan(L.explained_variance(np.arange(4.0), np.ones(4)))


def test_choose_target_kl_keeps_a_factor_of_two_on_both_sides():
    target, k = L.choose_target_kl([0.0, 1e-4, 3e-3, 5e-3, 4e-2, 5e-2])
    assert k == 2 and 2 * 1e-4 <= 1.5 * target <= 3e-3 / 2
    target, k = L.choose_target_kl([0.0, 2e-3, 4e-3, 7e-3, 8e-3])
    assert k == 1 and 0 < 1.5 * target <= 2e-3 / 2
    assert L.choose_target_kl([0.01, 0.011, 0.012, 0.013]) is None


def test_control_entry_points_reject_bad_arguments_without_a_gpu(library):
    for name in ("upkie_ppo_control_set", "upkie_ppo_update_begin", "upkie_ppo_minibatch_update_controlled",
                 "upkie_ppo_minibatch_gradient_controlled", "upkie_ppo_minibatch_apply_controlled", "upkie_ppo_explained_variance"):
        assert name in lib.EXPORTED_SYMBOLS and getattr(library, name) is not None
    block = (C.c_double * (abi.PPO_CTRL_WORDS + 1))()
    at = C.addressof(block)
    err = lambda: library.upkie_sim_last_error(None)  # noqa: E731
    assert library.upkie_ppo_control_set(None, 3e-4, 0.2, 0.0, 0.0, None) == abi.ERR_INVALID_ARGUMENT and b"null control" in err()
    assert library.upkie_ppo_control_set(at + 4, 3e-4, 0.2, 0.0, 0.0, None) == abi.ERR_INVALID_ARGUMENT and b"aligned" in err()
    for args in ((3e-4, 0.2, 0.0, -0.01), (3e-4, 0.0, 0.0, 0.0), (-1.0, 0.2, 0.0, 0.0), (3e-4, 0.2, -0.1, 0.0), (3e-4, 0.2, 0.0, math.nan),
                 (math.inf, 0.2, 0.0, 0.0)):
        assert library.upkie_ppo_control_set(at, *args, None) == abi.ERR_INVALID_ARGUMENT, args
        assert b"control" in err(), args
    assert library.upkie_ppo_update_begin(None, None) == abi.ERR_INVALID_ARGUMENT and b"null control" in err()
    assert library.upkie_ppo_update_begin(at + 4, None) == abi.ERR_INVALID_ARGUMENT and b"aligned" in err()
    shape = _shape(4, [64, 64], 1)
    cfg = abi.UpkiePpoConfig(0.2, 0.0, 0.0, 0.5, 0.5, 0.9, 0.999, 1e-5, 0, 0)
    buf = (C.c_float * 64)()
    d = (C.c_double * 2)()

    def update(control=at, size=32):
        return library.upkie_ppo_minibatch_update_controlled(C.byref(shape), C.byref(cfg), 64, 0, size, 32, buf, buf, buf, buf, buf, buf, buf, d, buf,
                                                             buf, buf, control, buf, buf, None)

    assert update(control=None) == abi.ERR_INVALID_ARGUMENT and b"null control" in err()
    assert update(control=at + 4) == abi.ERR_INVALID_ARGUMENT and b"aligned" in err()
    assert update(size=33) == abi.ERR_INVALID_ARGUMENT and b"minibatch" in err()
    grad = lambda control: library.upkie_ppo_minibatch_gradient_controlled(  # noqa: E731
        C.byref(shape), C.byref(cfg), 64, 0, 32, 64, 32, buf, buf, buf, buf, buf, buf, buf, d, buf, buf, buf, control, None)
    apply = lambda control, start=0: library.upkie_ppo_minibatch_apply_controlled(  # noqa: E731
        C.byref(shape), C.byref(cfg), start, 64, 32, buf, 2, buf, buf, buf, control, buf, buf, None)
    assert grad(None) == abi.ERR_INVALID_ARGUMENT and apply(None) == abi.ERR_INVALID_ARGUMENT and apply(at + 4) == abi.ERR_INVALID_ARGUMENT
    assert apply(at, start=-1) == abi.ERR_INVALID_ARGUMENT and b"minibatch_start" in err()
    ev = library.upkie_ppo_explained_variance
    assert ev(0, buf, buf, -1, None, 1, None, d, None) == abi.ERR_INVALID_ARGUMENT
    assert ev(8, buf, buf, 3, None, 1, None, d, None) == abi.ERR_INVALID_ARGUMENT
    assert ev(8, None, buf, -1, None, 1, None, d, None) == abi.ERR_INVALID_ARGUMENT and b"null" in err()
    assert ev(8, buf, buf, -1, None, 1, None, None, None) == abi.ERR_INVALID_ARGUMENT
    assert ev(8, buf, buf, 1, None, 2, d, d, None) == abi.ERR_INVALID_ARGUMENT
    if library.upkie_hip_device_count() == 0:
        assert library.upkie_ppo_control_set(at, 3e-4, 0.2, 0.0, 0.03, None) == abi.ERR_NO_DEVICE
        assert library.upkie_ppo_update_begin(at, None) == abi.ERR_NO_DEVICE and update() == abi.ERR_NO_DEVICE
        assert ev(8, buf, buf, -1, None, 1, None, d, None) == abi.ERR_NO_DEVICE


def _bare_policy():
    pol = MlpActorCritic.__new__(MlpActorCritic)  # (the shape is all the checks read: no device needed)
    pol.shape = _shape(4, [64, 64], 1)
    return pol


def test_trainer_checks_the_new_arguments_before_any_device_use():
    pol = _bare_policy()
    for kw in ({"target_kl": -0.01}, {"target_kl": 0.0}, {"target_kl": math.inf}):
        with pytest.raises(ValueError, match="target_kl"):
            PpoTrainer(pol, **kw)
    with pytest.raises(ValueError, match="clip_range"):
        PpoTrainer(pol, clip_range=lambda p: 0.2 * (p - 1.0))  # (evaluated at progress_remaining = 1)
    with pytest.raises(ValueError, match="clip_range_vf"):
        PpoTrainer(pol, clip_range_vf=lambda p: -1.0)
    with pytest.raises(ValueError, match="controlled"):
        PpoTrainer(pol, target_kl=0.03, controlled=False)
    with pytest.raises(ValueError, match="controlled"):
        PpoTrainer(pol, lr=lambda p: 3e-4 * p, controlled=False)


def test_set_progress_evaluates_the_callables_and_keeps_the_constants():
    """`set_progress` on a trainer whose device write is replaced by a recorder: callables are evaluated at
    progress_remaining, constants (and values set by hand) stay."""
    tr = PpoTrainer.__new__(PpoTrainer)
    tr._schedules = {"lr": lambda p: 1e-3 * p, "clip_range": 0.2, "clip_range_vf": lambda p: 0.5 * p}
    tr.controlled, tr._clip_range, tr._clip_range_vf, tr._target_kl, tr._lr = True, 0.2, 0.5, 0.03, 1e-3
    written = []
    tr._write_control = lambda lr: written.append((lr, tr._clip_range, tr._clip_range_vf, tr._target_kl))
    tr.set_progress(0.5)
    tr.set_target_kl(None)
    tr.set_clip_range(0.1, 0.3)
    tr.set_progress(0.25)
    assert written == [(5e-4, 0.2, 0.25, 0.03), (1e-3, 0.2, 0.25, None), (1e-3, 0.1, 0.3, None), (2.5e-4, 0.1, 0.125, None)]
    with pytest.raises(ValueError):
        tr.set_target_kl(-1.0)
    plain = PpoTrainer.__new__(PpoTrainer)
    plain._schedules, plain.controlled = {"lr": 3e-4, "clip_range": 0.2, "clip_range_vf": None}, False
    plain.set_progress(0.5)  # constants only: nothing to write
    assert plain.progress_remaining == 0.5
    with pytest.raises(UpkieRuntimeError, match="controlled"):
        plain.set_target_kl(0.01)
    with pytest.raises(UpkieRuntimeError, match="controlled"):
        plain.set_clip_range(0.1)


class _FakeEnv:
    num_envs = 8


class _FakeTrainer:
    def __init__(self):
        self.calls = []

    def set_progress(self, p):
        self.calls.append(("progress", p))

    def log(self):
        return {"loss": 1.0, "n_updates": 10 * sum(1 for c in self.calls if c[0] == "train")}


class _FakeEpisodes:
    def ep_rew_mean(self):
        return 2.5

    def ep_len_mean(self):
        return None


class _BookkeepingPpo(Ppo):
    def _setup(self):
        if self.trainer is None:
            self.trainer, self.episodes = _FakeTrainer(), _FakeEpisodes()

    def collect_rollouts(self):
        self.num_timesteps += self.n_steps * self.n_envs
        self.trainer.calls.append(("rollout", self.num_timesteps))

    def train(self):
        self.trainer.calls.append(("train", self.trainer.calls[-1][1]))


def test_learn_follows_sb3s_bookkeeping():
    model = _BookkeepingPpo(_FakeEnv(), object(), n_steps=4)  # 32 steps per iteration
    seen = []
    model.learn(100, callback=lambda m, rec: seen.append(rec), log_interval=2)  # SB3: whole iterations until num_timesteps >= total
    assert model.num_timesteps == 128 and model.iterations == 4
    calls = model.trainer.calls
    assert [c for c in calls if c[0] == "progress"] == [("progress", 1.0 - n / 100.0) for n in (32, 64, 96, 128)]
    assert [c[0] for c in calls] == ["rollout", "progress", "train"] * 4, "progress_remaining is set after the rollout, before the update"
    assert [rec is not None for rec in seen] == [False, True, False, True]
    assert seen[3] == {"train/loss": 1.0, "train/n_updates": 40, "rollout/ep_rew_mean": 2.5, "rollout/ep_len_mean": None,
                       "time/total_timesteps": 128, "time/iterations": 4}
    assert model.records == [seen[1], seen[3]]
    # a callback that returns False ends training (None does not); continuing adds to the total, as SB3's _setup_learn
    model.learn(1000, callback=lambda m, rec: m.iterations < 2)
    assert model.iterations == 2 and model.num_timesteps == 64
    model.learn(64, reset_num_timesteps=False)
    assert model.total_timesteps == 128 and model.num_timesteps == 128 and model.iterations == 4
    assert model.trainer.calls[-2] == ("progress", 0.0)
    with pytest.raises(ValueError):
        Ppo(_FakeEnv(), object(), n_steps=0)


# ---------------------------------------------------------------- Ppo.save / Ppo.load: what the file holds
class _SavedPpo(Ppo):
    """`Ppo` whose stages are host stand-ins: every tensor a stage owns is filled with its own number (times the
    stand-in env's ``scale``, so that two sets of objects differ everywhere)."""

    def _setup(self):
        if self.buffer is not None:
            return
        from upkie_amd.episodes import EpisodeStatistics

        scale = self.env.scale
        f = filler(range(1, 100), scale)
        self.buffer, self.device, self.normalizer = object(), torch.device("cpu"), None
        self.trainer = stage(PpoTrainer, m=f(6), v=f(6), control=f(abi.PPO_CTRL_WORDS, dtype=torch.float64), generator=torch.Generator(),
                              _clip_range=0.2 * scale, _clip_range_vf=None, _target_kl=0.03 * scale, _lr=1e-3 * scale,
                              progress_remaining=1.0, sync_modules=lambda: None)
        self.trainer.generator.manual_seed(5 * scale)
        self.episodes = stage(EpisodeStatistics, ep_return=f(2, dtype=torch.float64), ep_length=f(2, dtype=torch.int32),
                               ring_return=f(3, dtype=torch.float64), ring_length=f(3, dtype=torch.int32), counters=f(3, dtype=torch.int64),
                               means=f(2, dtype=torch.float64))
        self._starts, self._obs = f(2, dtype=torch.uint8), f(2, 4)


STAGE_TENSORS = ["calls", "control", "env.final_obs", "env.observation", "env.reward", "env.state", "env.terminated", "env.truncated", "ep_counters",
                 "ep_length", "ep_means", "ep_return", "m", "packed", "ring_length", "ring_return", "starts", "v"]
PIPELINE_TENSORS = ["pipeline.calls", "pipeline.observation", "pipeline.prev_command"]
REWARD_TENSORS = ["reward.finished", "reward.prev_action", "reward.term_last", "reward.term_sum"]


@pytest.mark.parametrize("pipeline,reward,names", [(False, False, STAGE_TENSORS), (True, False, STAGE_TENSORS + PIPELINE_TENSORS),
                                                   (False, True, STAGE_TENSORS + REWARD_TENSORS)])
def test_save_writes_these_names_and_load_puts_them_back(tmp_path, monkeypatch, pipeline, reward, names):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: None)
    path = str(tmp_path / "ppo.pt")
    env, policy, kwargs = saved_parts(1, pipeline, reward)
    model = _SavedPpo(env, policy, n_steps=4, **kwargs)
    model._setup()
    model.num_timesteps, model.iterations, model.total_timesteps, model.progress_remaining = 24, 3, 80, 0.7
    model.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(sd) == ["counters", "generator", "normalizer", "sizes", "tensors", "trainer"]
    assert sorted(sd["tensors"]) == sorted(names)
    assert sd["trainer"] == {"clip_range": 0.2, "clip_range_vf": None, "target_kl": 0.03, "lr": 1e-3}
    assert sd["counters"] == {"num_timesteps": 24, "iterations": 3, "total_timesteps": 80, "progress_remaining": 0.7, "policy_seed": 7}
    assert sd["sizes"] == {"n_envs": 2, "n_steps": 4} and sd["normalizer"] is None
    # every name holds the tensor of the stage that owns it
    tr, ep = model.trainer, model.episodes
    owners = {"packed": policy.packed, "calls": policy.calls, "m": tr.m, "v": tr.v, "control": tr.control, "starts": model._starts,
              "ep_return": ep.ep_return, "ep_length": ep.ep_length, "ring_return": ep.ring_return, "ring_length": ep.ring_length,
              "ep_counters": ep.counters, "ep_means": ep.means, "env.state": env.sim.state, "env.reward": env.sim.reward,
              "env.terminated": env.sim.terminated, "env.truncated": env.sim.truncated, "env.observation": model._obs, "env.final_obs": env._final_obs}
    owners.update({f"pipeline.{k}": v for k, v in (kwargs["pipeline"].state_tensors() if pipeline else {}).items()})
    owners.update({f"reward.{k}": v for k, v in (kwargs["reward"].state_tensors() if reward else {}).items()})
    assert owners.keys() == sd["tensors"].keys() and all(torch.equal(sd["tensors"][k], v) and sd["tensors"][k].dtype == v.dtype for k, v in owners.items())
    # into fresh objects holding other numbers
    env2, policy2, kwargs2 = saved_parts(2, pipeline, reward)
    loaded = _SavedPpo.load(path, env2, policy2, n_steps=4, **kwargs2)
    assert all(torch.equal(sd["tensors"][k], v) for k, v in loaded._state_tensors().items()) and loaded._state_tensors().keys() == owners.keys()
    assert torch.equal(policy2.packed, policy.packed) and torch.equal(loaded.episodes.counters, ep.counters) and policy2.seed == 7
    tr2 = loaded.trainer
    assert (tr2._clip_range, tr2._clip_range_vf, tr2._target_kl, tr2._lr, tr2.progress_remaining) == (0.2, None, 0.03, 1e-3, 0.7)
    assert torch.equal(tr2.generator.get_state(), tr.generator.get_state())
    assert (loaded.num_timesteps, loaded.iterations, loaded.total_timesteps, loaded.progress_remaining) == (24, 3, 80, 0.7)
    if not reward:  # a file without the reward's tensors does not load into a Ppo with one
        env3, policy3, kwargs3 = saved_parts(2, pipeline, True)
        with pytest.raises(ValueError, match="the file has no reward.prev_action"):
            _SavedPpo.load(path, env3, policy3, n_steps=4, **kwargs3)
