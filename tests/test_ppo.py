"""The PPO update (upkie_amd.ppo, csrc/ppo.hpp) without a GPU: the fp64 twin of tests/ppo_reference.py against torch
autograd of the literal Stable-Baselines3 expression, the trainable-word mask, the workspace size and the entry points'
argument checks."""

import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import mlp_reference as MR
from tests import ppo_reference as R
from upkie_amd import abi, lib
from upkie_amd.exceptions import UpkieRuntimeError
from upkie_amd.policies import MlpActorCritic, mlp_shape, pack_index
from upkie_amd.ppo import PpoTrainer, trainable_offset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def library():
    lib.build()
    return lib.load()


def _dims(D, widths, out):
    return [(w, n) for w, n in zip(list(widths) + [out], [D] + list(widths))]


def _shape(D, widths, A, act="tanh", normalize=False, critic=True):
    return mlp_shape(_dims(D, widths, A), _dims(D, widths, 1) if critic else [], act, normalize, 3.0)


def _modules(D, widths, A, act, seed):
    torch.manual_seed(seed)
    tower = lambda out: torch.nn.Sequential(*sum([[torch.nn.Linear(n, w), torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU()]  # noqa: E731
                                                  for w, n in zip(widths, [D] + widths[:-1])], []), torch.nn.Linear(widths[-1], out)).double()
    return tower(A), tower(1)


def _sources(actor, critic, log_std, D, A, mean, std):
    src = [mean, std, -np.ones(A), np.ones(A), log_std.detach().numpy().copy()]
    for seq in (actor, critic):
        for m in seq:
            if isinstance(m, torch.nn.Linear):
                src += [m.weight.detach().numpy().copy(), m.bias.detach().numpy().copy()]
    return src


def _torch_sb3(actor, critic, log_std, x, actions, old_values, old_log_prob, adv, returns, c):
    """SB3 PPO.train's minibatch, literally, in float64: the loss and its gradient (autograd), clip_grad_norm_, Adam."""
    params = [log_std] + [p for seq in (actor, critic) for m in seq if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]
    if c["normalize_advantage"] and len(adv) > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    mean = actor(x)
    dist = torch.distributions.Normal(mean, torch.ones_like(mean) * log_std.exp())
    log_prob = dist.log_prob(actions).sum(dim=1)
    entropy = dist.entropy().sum(dim=1)
    values = critic(x).flatten()
    ratio = torch.exp(log_prob - old_log_prob)
    policy_loss_1 = adv * ratio
    policy_loss_2 = adv * torch.clamp(ratio, 1 - c["clip_range"], 1 + c["clip_range"])
    policy_loss = -torch.min(policy_loss_1, policy_loss_2).mean()
    if c["clip_range_vf"] is None:
        values_pred = values
    else:
        values_pred = old_values + torch.clamp(values - old_values, -c["clip_range_vf"], c["clip_range_vf"])
    value_loss = torch.nn.functional.mse_loss(returns, values_pred)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss + c["ent_coef"] * entropy_loss + c["vf_coef"] * value_loss
    opt = torch.optim.Adam(params, lr=c["lr"], eps=1e-5)
    opt.zero_grad()
    loss.backward()
    grads = [p.grad.clone() for p in params]
    norm = torch.nn.utils.clip_grad_norm_(params, c["max_grad_norm"])
    opt.step()
    with torch.no_grad():
        log_ratio = log_prob - old_log_prob
        kl = torch.mean((torch.exp(log_ratio) - 1) - log_ratio)
        frac = torch.mean((torch.abs(ratio - 1) > c["clip_range"]).double())
    stats = [policy_loss.item(), value_loss.item(), entropy_loss.item(), loss.item(), kl.item(), frac.item(), float(norm)]
    state = [(opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in params]
    return np.array(stats), [g.numpy() for g in grads], [p.detach().numpy().copy() for p in params], state


# (B, D, widths, A, activation, config overrides, first minibatch: old log-probs are the current ones -> every ratio 1)
CASES = [
    (64, 4, [64, 64], 1, "tanh", {}, True),
    (50, 6, [40, 24], 3, "relu", {"clip_range_vf": 0.1, "ent_coef": 0.01}, False),
    (33, 5, [16], 2, "tanh", {"ent_coef": -0.02, "clip_range": 0.1}, False),
    (1, 3, [16, 8], 2, "relu", {}, False),  # one sample: no advantage normalisation
    (20, 7, [32], 5, "tanh", {"normalize_advantage": False, "clip_range_vf": 0.3, "max_grad_norm": 1e9}, True),
]


@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}-A{c[3]}-{c[4]}" for c in CASES])
def test_fp64_twin_is_torch_autograd_of_sb3(case):
    B, D, widths, A, act, over, first = case
    c = dict(R.DEFAULTS, **over)
    rng = np.random.default_rng(B)
    actor, critic = _modules(D, widths, A, act, seed=B)
    log_std = torch.tensor(rng.normal(-0.5, 0.3, size=A), requires_grad=True)
    mean, std = rng.normal(0, 0.3, D), rng.uniform(0.5, 2.0, D)
    shape = _shape(D, widths, A, act, normalize=True)
    obs = rng.normal(0, 2.0, size=(B, D))
    src = _sources(actor, critic, log_std, D, A, mean, std)
    x = MR.normalize(shape, src, obs)
    with torch.no_grad():
        mu = actor(torch.as_tensor(x)).numpy()
        v = critic(torch.as_tensor(x)).numpy()[:, 0]
    actions = mu + np.exp(log_std.detach().numpy()) * rng.normal(size=(B, A))
    if first:
        old_lp = MR.log_prob(actions, mu, log_std.detach().numpy())
    else:
        old_lp = MR.log_prob(actions, mu, log_std.detach().numpy()) + rng.normal(0, 0.2, B)
    old_v = v + rng.normal(0, 0.2, B)
    adv, ret = rng.normal(0, 1.0, B), v + rng.normal(0, 1.0, B)

    stats, grads, ratio = R.minibatch(shape, src, obs, actions, old_v, old_lp, adv, ret, **over)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    want_stats, want_grads, want_params, want_state = _torch_sb3(actor, critic, log_std, t(x), t(actions), t(old_v), t(old_lp), t(adv), t(ret), c)
    if first:
        assert np.all(np.abs(ratio - 1.0) < 1e-12), "the first minibatch ties every sample at ratio 1"
    else:
        lo, hi = 1 - c["clip_range"], 1 + c["clip_range"]
        assert (ratio < lo).any() or (ratio > hi).any() or B == 1, "some samples clipped"
    for g, w in zip(grads, want_grads):
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(w).max()))
    np.testing.assert_allclose(stats, want_stats, rtol=1e-12, atol=1e-12)
    params, m, vv, step = R.adam_step(R.trainable(shape, src), grads, [0 * g for g in grads], [0 * g for g in grads], 0,
                                      c["max_grad_norm"], c["lr"])
    assert step == 1
    for p, w, mm, vs, (wm, wv) in zip(params, want_params, m, vv, want_state):
        np.testing.assert_allclose(p, w, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(mm, wm.numpy(), rtol=1e-12, atol=1e-18)
        np.testing.assert_allclose(vs, wv.numpy(), rtol=1e-12, atol=1e-24)


def test_surrogate_gradient_at_exact_ties_and_clip_bounds():
    """torch.minimum's half / half split where the two surrogates tie and clamp's pass-through at exactly 1 +- c."""
    c = 0.2
    ratio = torch.tensor([1.0, 1 - c, 1 + c, 1 - c, 1 + c, 0.5, 1.5, 1.1], dtype=torch.float64, requires_grad=True)
    adv = torch.tensor([0.7, 1.3, -0.4, -2.0, 0.9, 1.0, -1.0, 0.0], dtype=torch.float64)
    torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - c, 1 + c)).sum().backward()
    got = R.surrogate_grad(adv.numpy(), ratio.detach().numpy(), c)
    np.testing.assert_array_equal(got, ratio.grad.numpy())
    assert got[0] == 0.7 and got[1] == 1.3 and got[3] == -2.0  # inside or at a bound: ties, the clamp passes


def test_trainable_mask_is_the_parameters_pack_positions():
    for D, widths, A, act in ((4, [64, 64], 1, "tanh"), (6, [40, 24], 3, "relu"), (30, [256, 256, 128], 36, "tanh"), (17, [48, 5], 64, "relu")):
        shape = _shape(D, widths, A, act, normalize=True)
        sizes = [D, D, A, A, A]
        for w, n in _dims(D, widths, A) + _dims(D, widths, 1):
            sizes += [w * n, w]
        index = pack_index(shape, sizes)
        zero = sum(sizes)
        fixed_end = 4 * 0 + sum(sizes[:4])
        off = trainable_offset(shape)
        assert off == MR._layout(shape)["log_std"]
        mask = (np.arange(index.size) >= off) & (index != zero)
        params = (index >= fixed_end) & (index != zero)
        np.testing.assert_array_equal(mask, params)
        assert not ((index[:off] >= fixed_end) & (index[:off] != zero)).any(), "no parameter before the offset"
        assert set(index[off:][index[off:] != zero]) == set(range(fixed_end, zero)), "every parameter word is past it"


def test_workspace_is_bounded_needs_no_device_and_rejects_bad_shapes(library):
    big = _shape(256, [256, 256, 256, 256], 64)
    sizes = []
    for spec in ((4, [64, 64], 1), (4, [256, 256], 1), (256, [256] * 4, 64), (1, [1], 1), (255, [200, 17, 256], 63), (30, [256, 256, 128], 36)):
        shape = _shape(*spec)
        for mb in (1, 17, 4096, 131072, 1 << 22, (1 << 31) - 1):
            n = library.upkie_ppo_workspace_bytes(C.byref(shape), mb)
            assert 0 < n <= 64 << 20, (spec, mb, n)
            sizes.append(n)
    assert library.upkie_ppo_workspace_bytes(C.byref(big), 1 << 20) <= 64 << 20
    small = _shape(4, [64, 64], 1)
    assert library.upkie_ppo_workspace_bytes(C.byref(small), 16) < library.upkie_ppo_workspace_bytes(C.byref(small), 131072)
    assert library.upkie_ppo_workspace_bytes(C.byref(small), 0) == abi.ERR_INVALID_ARGUMENT
    assert b"max_minibatch" in library.upkie_sim_last_error(None)
    no_critic = _shape(4, [64, 64], 1, critic=False)
    assert library.upkie_ppo_workspace_bytes(C.byref(no_critic), 64) == abi.ERR_INVALID_ARGUMENT
    assert b"critic" in library.upkie_sim_last_error(None)
    bad = _shape(4, [64], 1)
    bad.actor_widths[0] = 300
    assert library.upkie_ppo_workspace_bytes(C.byref(bad), 64) == abi.ERR_INVALID_ARGUMENT
    assert library.upkie_ppo_workspace_bytes(None, 64) == abi.ERR_INVALID_ARGUMENT


def test_entry_points_reject_bad_arguments_without_a_gpu(library):
    with open(os.path.join(ROOT, "include", "upkie_hip.h")) as fh:
        declared = set(re.findall(r"\b(upkie_[a-z_]+)\s*\(", fh.read()))
    for name in ("upkie_ppo_workspace_bytes", "upkie_ppo_advantage_stats", "upkie_ppo_minibatch_update"):
        assert name in declared and name in lib.EXPORTED_SYMBOLS and getattr(library, name) is not None
    assert library.upkie_hip_struct_bytes(10) == C.sizeof(abi.UpkiePpoConfig) and abi.STRUCT_IDS[10] is abi.UpkiePpoConfig
    shape = _shape(4, [64, 64], 1)
    cfg = abi.UpkiePpoConfig(0.2, 0.0, 0.0, 0.5, 0.5, 0.9, 0.999, 1e-5, 0, 0)
    buf = (C.c_float * 64)()
    d = (C.c_double * 2)()

    def update(cfg=cfg, total=64, start=0, size=32, max_mb=32, shape=shape, ptr=buf):
        return library.upkie_ppo_minibatch_update(C.byref(shape), C.byref(cfg), total, start, size, max_mb, buf, buf, buf, buf, buf, buf, buf, d, buf,
                                                  buf, buf, d, buf, ptr, None)

    for kwargs, word in (({"size": 0}, b"minibatch"), ({"start": 40}, b"minibatch"), ({"size": 33}, b"minibatch"), ({"start": -1}, b"minibatch"),
                         ({"ptr": None}, b"null"), ({"shape": _shape(4, [64, 64], 1, critic=False)}, b"critic")):
        assert update(**kwargs) == abi.ERR_INVALID_ARGUMENT, kwargs
        assert word in library.upkie_sim_last_error(None), kwargs
    for field, value in (("clip_range", 0.0), ("max_grad_norm", -1.0), ("adam_beta1", 1.0), ("adam_eps", 0.0), ("vf_coef", math.inf)):
        bad = abi.UpkiePpoConfig.from_buffer_copy(cfg)
        setattr(bad, field, value)
        assert update(cfg=bad) == abi.ERR_INVALID_ARGUMENT and b"config" in library.upkie_sim_last_error(None), field
    assert library.upkie_ppo_advantage_stats(0, 4, buf, buf, 1, d, None) == abi.ERR_INVALID_ARGUMENT
    assert library.upkie_ppo_advantage_stats(8, 4, None, buf, 1, d, None) == abi.ERR_INVALID_ARGUMENT
    if library.upkie_hip_device_count() == 0:
        assert update() == abi.ERR_NO_DEVICE and b"no HIP device" in library.upkie_sim_last_error(None)
        assert library.upkie_ppo_advantage_stats(8, 4, buf, buf, 1, d, None) == abi.ERR_NO_DEVICE


def test_a_library_built_before_the_ppo_update_still_loads():
    """An older build (no PPO entry points) answers -1 for UpkiePpoConfig: accepted. One that exports the entry point
    must report the struct's size."""
    sizes = {which: C.sizeof(cls) for which, cls in abi.STRUCT_IDS.items()}
    cases = "".join(f"    case {w}: return {n};\n" for w, n in sizes.items() if w != 10)
    stub = "#include <stdint.h>\nint64_t upkie_hip_struct_bytes(int which) {\n  switch (which) {\n" + cases + "    default: return -1;\n  }\n}\n"
    with tempfile.TemporaryDirectory() as tmp:
        for exports_entry in (False, True):
            src, so = os.path.join(tmp, f"stub{int(exports_entry)}.c"), os.path.join(tmp, f"libstub{int(exports_entry)}.so")
            with open(src, "w") as f:
                f.write(stub + "int upkie_mlp_actor_critic(void) { return -1; }\n"
                        + ("int upkie_ppo_minibatch_update(void) { return -1; }\n" if exports_entry else ""))
            subprocess.run(["gcc", "-shared", "-fPIC", src, "-o", so], check=True)
            older = C.CDLL(so)
            if exports_entry:
                with pytest.raises(UpkieRuntimeError, match="UpkiePpoConfig"):
                    lib._check_struct_sizes(older)
            else:
                lib._check_struct_sizes(older)


def test_trainer_refuses_a_policy_without_a_critic():
    pol = MlpActorCritic.__new__(MlpActorCritic)  # (the shape is all the check reads: no device needed)
    pol.shape = _shape(4, [64, 64], 1, critic=False)
    with pytest.raises(ValueError, match="critic"):
        PpoTrainer(pol)
    with pytest.raises(TypeError):
        PpoTrainer(object())
