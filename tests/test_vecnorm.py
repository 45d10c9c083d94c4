"""The running normaliser (upkie_amd.normalize.RunningNormalizer, csrc/vecnorm.hpp) without a GPU: the fp64 twin the
GPU tests compare against (tests/test_vecnorm_gpu.py), argument checks, the exported symbols, saving and loading, and
where the kernel writes a policy's live statistics."""

import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import vecnorm_reference as R
from upkie_amd import abi, lib
from upkie_amd.exceptions import UpkieRuntimeError
from upkie_amd.normalize import RunningNormalizer, packed_offsets
from upkie_amd.policies import pack_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def library():
    lib.build()
    return lib.load()


def test_twin_merge_is_the_moments_of_the_concatenation():
    rng = np.random.default_rng(0)
    rms = R.RunningMeanStd((3,), epsilon=0.0)
    rms.count = 0.0
    chunks = [rng.normal(loc=[1e3, 0.0, -5.0], scale=[0.1, 1.0, 3.0], size=(n, 3)).astype(np.float32) for n in (1, 7, 64, 300)]
    for x in chunks:
        rms.update(x)
    data = np.concatenate(chunks).astype(np.float64)
    assert rms.count == data.shape[0]
    np.testing.assert_allclose(rms.mean, data.mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(rms.var, data.var(axis=0), rtol=1e-9)


def _pooled(values, eps=1e-4):
    """RunningMeanStd(eps) after updates with all `values`: the initial state is a pseudo-batch of count eps, mean 0,
    variance 1 (plain Python, not the twin's merge)."""
    n = eps + len(values)
    mean = sum(values) / n
    m2 = eps * 1.0 + eps * mean * mean + sum((v - mean) ** 2 for v in values)
    return mean, m2 / n, n


def test_twin_on_a_hand_worked_sequence():
    """3 envs, 4 steps, gamma 0.5: env 1 ends at step 1 and env 0 at step 3; their returns restart from 0."""
    twin = R.VecNormalizeTwin(3, 2, gamma=0.5, clip_reward=100.0)
    obs = [np.array([[1, 0], [2, 0], [3, 1]], np.float32) * (t + 1) for t in range(4)]
    rewards = [[1, 2, 0], [1, 0, 4], [2, 2, 2], [0, 1, 0]]
    dones = [[0, 0, 0], [0, 1, 0], [0, 0, 0], [1, 0, 0]]
    # returns by hand: r_t = 0.5 r_{t-1} + reward_t, zeroed after a done step
    seen = [[1, 2, 0], [1.5, 1, 4], [2.75, 2, 4], [1.375, 2, 2]]
    after = [[1, 2, 0], [1.5, 0, 4], [2.75, 2, 4], [0, 2, 2]]
    twin.reset(np.zeros((3, 2), np.float32))
    rows = [[0.0, 0.0]] * 3
    for t in range(4):
        nobs, r, starts = twin.step(obs[t], np.array(rewards[t], np.float32), np.array(dones[t], bool), np.zeros(3, bool))
        np.testing.assert_array_equal(twin.returns, after[t])
        np.testing.assert_array_equal(starts, dones[t])
        mean, var, count = _pooled([v for step in seen[: t + 1] for v in step])
        assert twin.ret_rms.count == pytest.approx(count, rel=1e-15)
        assert twin.ret_rms.mean == pytest.approx(mean, rel=1e-12)
        assert twin.ret_rms.var == pytest.approx(var, rel=1e-12)
        np.testing.assert_allclose(r, np.array(rewards[t]) / math.sqrt(var + 1e-8), rtol=1e-6)
        rows = rows + [list(map(float, o)) for o in obs[t]]
        for d in range(2):
            m, v, n = _pooled([row[d] for row in rows])
            assert twin.obs_rms.mean[d] == pytest.approx(m, rel=1e-12, abs=1e-15)
            assert twin.obs_rms.var[d] == pytest.approx(v, rel=1e-12)
        np.testing.assert_allclose(nobs, np.clip((obs[t] - twin.obs_rms.mean) / np.sqrt(twin.obs_rms.var + 1e-8), -10, 10), rtol=1e-6, atol=1e-6)
    assert twin.obs_rms.count == pytest.approx(1e-4 + 15)  # (reset's 3 rows and 4 steps of 3)
    twin.reset(obs[0])
    np.testing.assert_array_equal(twin.returns, 0.0)


def test_twin_modes():
    x = np.arange(6, dtype=np.float32).reshape(3, 2)
    frozen = R.VecNormalizeTwin(3, 2, training=False)
    _, r, _ = frozen.step(x, np.ones(3, np.float32), np.zeros(3), np.zeros(3))
    assert frozen.obs_rms.count == 1e-4 and frozen.ret_rms.count == 1e-4 and np.all(frozen.returns == 0)
    np.testing.assert_array_equal(r, np.float32(1 / math.sqrt(1 + 1e-8)))
    raw = R.VecNormalizeTwin(3, 2, norm_reward=False, norm_obs=False)
    nobs, r, _ = raw.step(x, np.full(3, 7, np.float32), np.zeros(3), np.zeros(3))
    np.testing.assert_array_equal(r, 7.0)
    np.testing.assert_array_equal(nobs, x)
    assert raw.ret_rms.count == pytest.approx(3 + 1e-4) and raw.obs_rms.count == 1e-4


def test_argument_checks_and_no_cpu_fallback(library):
    for bad in (dict(num_envs=0, obs_dim=4), dict(num_envs=4, obs_dim=0), dict(num_envs=4, obs_dim=257), dict(num_envs=4, obs_dim=4, gamma=1.5),
                dict(num_envs=4, obs_dim=4, epsilon=0.0), dict(num_envs=4, obs_dim=4, clip_obs=-1.0), dict(num_envs=4, obs_dim=4, clip_reward=0.0)):
        with pytest.raises(ValueError):
            RunningNormalizer(device="cpu", **bad)
    cpu = RunningNormalizer(4, 3, device="cpu")
    with pytest.raises(UpkieRuntimeError, match="no CPU fallback"):
        cpu.step(torch.zeros(4, 3), torch.zeros(4))
    with pytest.raises(UpkieRuntimeError, match="no CPU fallback"):
        cpu.normalize_reward(torch.zeros(4))
    with pytest.raises(UpkieRuntimeError, match="dict or tuple"):
        cpu.step({"a": torch.zeros(4, 3)}, torch.zeros(4))

    class Sharded:
        world_size, num_envs = 2, 4

    with pytest.raises(UpkieRuntimeError, match="ShardedVecEnv"):
        RunningNormalizer.for_env(Sharded())

    # the C entry point: argument checks come first, then the device check
    d = (C.c_double * 16)()
    f = (C.c_float * 16)()
    args = lambda n, dim, flags, ws: (n, dim, f, f, None, None, d, d, d, ws, flags, 0.99, 1e-8, 10.0, 10.0, f, f, None, None, f, None, None)  # noqa: E731
    assert library.upkie_vecnorm_step(*args(0, 3, 7, d)) == abi.ERR_INVALID_ARGUMENT
    assert library.upkie_vecnorm_step(*args(4, 3, 64, d)) == abi.ERR_INVALID_ARGUMENT
    assert b"flags" in library.upkie_sim_last_error(None)
    assert library.upkie_vecnorm_step(*args(4, 3, 7, None)) == abi.ERR_INVALID_ARGUMENT
    assert b"workspace" in library.upkie_sim_last_error(None)
    if library.upkie_hip_device_count() == 0:
        assert library.upkie_vecnorm_step(*args(4, 3, 7, d)) == abi.ERR_NO_DEVICE
        assert b"no HIP device" in library.upkie_sim_last_error(None)


def test_symbols_in_header_list_and_library(library):
    with open(os.path.join(ROOT, "include", "upkie_hip.h")) as fh:
        declared = set(re.findall(r"\b(upkie_[a-z_]+)\s*\(", fh.read()))
    for name in ("upkie_vecnorm_workspace_bytes", "upkie_vecnorm_step"):
        assert name in declared and name in lib.EXPORTED_SYMBOLS and getattr(library, name) is not None
    # callable without a GPU: one partial of (mean, M2) per column of launch A's blocks, behind the 256-byte ticket
    assert library.upkie_vecnorm_workspace_bytes(4096, 4) == 256 + 16 * 2 * 5 * 8
    assert library.upkie_vecnorm_workspace_bytes(1, 3) == 256 + 2 * 4 * 8
    big = library.upkie_vecnorm_workspace_bytes(1 << 20, 256)
    assert 0 < big <= 256 + 64 * 1024, "the partials stay <= 64 KB at large obs_dim"
    assert library.upkie_vecnorm_workspace_bytes(1 << 20, 4) == 256 + 256 * 2 * 5 * 8
    assert library.upkie_vecnorm_workspace_bytes(0, 4) == abi.ERR_INVALID_ARGUMENT
    assert b"obs_dim" in library.upkie_sim_last_error(None)
    assert library.upkie_vecnorm_workspace_bytes(4, 300) == abi.ERR_INVALID_ARGUMENT


class _Rms:
    def __init__(self, mean, var, count):
        self.mean, self.var, self.count = mean, var, count


class _FakeVecNormalize:
    """The attributes of Stable-Baselines3's VecNormalize that from_sb3 / to_sb3 read and write."""

    def __init__(self, n, d, seed):
        rng = np.random.default_rng(seed)
        self.obs_rms = _Rms(rng.normal(size=d), rng.uniform(0.1, 5.0, size=d), 1234.5678)
        self.ret_rms = _Rms(np.float64(rng.normal()), np.float64(rng.uniform(0.5, 2.0)), 987.654321)
        self.returns = rng.normal(size=n)
        self.gamma, self.epsilon, self.clip_obs, self.clip_reward = 0.95, 1e-7, 5.0, 3.0
        self.norm_obs, self.norm_reward, self.training = True, False, False


def test_state_dict_and_sb3_round_trips_are_bit_exact(library):
    src = _FakeVecNormalize(5, 3, seed=1)
    norm = RunningNormalizer.from_sb3(src, device="cpu")
    assert (norm.num_envs, norm.obs_dim, norm.gamma, norm.epsilon, norm.clip_obs, norm.clip_reward) == (5, 3, 0.95, 1e-7, 5.0, 3.0)
    assert (norm.norm_obs, norm.norm_reward, norm.training) == (True, False, False)
    np.testing.assert_array_equal(norm.obs_mean.numpy(), src.obs_rms.mean)
    np.testing.assert_array_equal(norm.obs_var.numpy(), src.obs_rms.var)
    np.testing.assert_array_equal(norm.returns.numpy(), src.returns)
    assert float(norm.obs_count) == src.obs_rms.count and float(norm.ret_var) == src.ret_rms.var
    np.testing.assert_array_equal(norm.obs_mean_f32.numpy(), src.obs_rms.mean.astype(np.float32))
    np.testing.assert_array_equal(norm.obs_std_f32.numpy(), np.sqrt(src.obs_rms.var + 1e-7).astype(np.float32))

    dst = _FakeVecNormalize(5, 3, seed=2)
    dst.norm_reward, dst.training, dst.gamma = True, True, 0.5
    norm.to_sb3(dst)
    for a, b in ((dst.obs_rms, src.obs_rms), (dst.ret_rms, src.ret_rms)):
        np.testing.assert_array_equal(a.mean, b.mean)
        np.testing.assert_array_equal(a.var, b.var)
        assert a.count == b.count
    np.testing.assert_array_equal(dst.returns, src.returns)
    assert (dst.gamma, dst.epsilon, dst.clip_obs, dst.clip_reward, dst.norm_obs, dst.norm_reward, dst.training) == (
        0.95, 1e-7, 5.0, 3.0, True, False, False)
    with pytest.raises(ValueError):
        norm.to_sb3(_FakeVecNormalize(6, 3, seed=3))

    sd = norm.state_dict()
    other = RunningNormalizer(5, 3, device="cpu")
    other.load_state_dict(sd)
    for key, value in other.state_dict().items():
        if isinstance(value, torch.Tensor):
            assert torch.equal(value, sd[key]), key
        else:
            assert value == sd[key], key
    assert torch.equal(other.obs_stats, norm.obs_stats) and torch.equal(other.ret_stats, norm.ret_stats)
    with pytest.raises(ValueError):
        RunningNormalizer(5, 4, device="cpu").load_state_dict(sd)

    dict_obs = _FakeVecNormalize(5, 3, seed=4)
    dict_obs.obs_rms = {"a": dict_obs.obs_rms}
    with pytest.raises(UpkieRuntimeError, match="dict observations"):
        RunningNormalizer.from_sb3(dict_obs, device="cpu")


# the MLP shapes of tests/test_mlp_policy.py: (obs_dim, actor widths, act_dim, critic widths, activation)
SHAPES = [
    (4, [64, 64], 1, [64, 64], "tanh"),
    (6, [64, 64], 2, [64, 64], "relu"),
    (30, [256, 256, 128], 36, [256, 256, 128], "tanh"),
    (3, [16], 2, [16], "relu"),
    (5, [7, 33, 20, 1], 17, [], "tanh"),
    (17, [48], 64, [3, 256, 5, 9], "relu"),
]


@pytest.mark.parametrize("spec", SHAPES, ids=[f"obs{s[0]}-{s[4]}" for s in SHAPES])
def test_mirror_offsets_are_the_packed_obs_mean_and_obs_std(spec):
    from upkie_amd.policies import mlp_shape

    D, aw, A, cw, act = spec
    dims = lambda widths, out: [(w, n) for w, n in zip(list(widths) + [out], [D] + list(widths))]  # noqa: E731
    shape = mlp_shape(dims(aw, A), dims(cw, 1) if cw else [], act, True)
    sizes = [D, D, A, A, A]
    for w, n in dims(aw, A) + (dims(cw, 1) if cw else []):
        sizes += [w * n, w]
    index = pack_index(shape, sizes)
    mean_at, std_at = packed_offsets(D)
    np.testing.assert_array_equal(index[mean_at: mean_at + D], np.arange(D))  # source 0: obs_mean
    np.testing.assert_array_equal(index[std_at: std_at + D], D + np.arange(D))  # source 1: obs_std
    assert not np.isin(np.arange(2 * D), np.delete(index, np.r_[mean_at: mean_at + D, std_at: std_at + D])).any()
