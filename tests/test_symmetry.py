"""Mirror symmetry of the PPO update on the host: the fp64 twin (tests/symmetry_reference.py) against torch autograd, the
header against abi.py, every refusal by name, the Gyropod table against the fp64 oracle, and the input conditions of
tests/test_symmetry_gpu.py on every row of tests/mlp_shapes.MATRIX -- including that those inputs tell each one-line
mistake (`symmetry_reference.MUTATIONS`) from the feature."""

import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import asymmetric_reference as AR
from tests import asymmetric_shapes as AS
from tests import mlp_reference as R
from tests import mlp_shapes as S
from tests import ppo_reference as PR
from tests import symmetry_reference as SR
from upkie_amd import abi, lib
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import MIRROR_STAT_NAMES, Ppo, PpoTrainer
from upkie_amd.symmetry import GYROPOD_ACT_SIGN, GYROPOD_OBS_SIGN, MirrorSymmetry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(ent_coef=0.01, clip_range_vf=0.2, max_grad_norm=1e9)
COEF = 0.5


@pytest.fixture(scope="module")
def library():
    lib.build()
    return lib.load()


# ---------------------------------------------------------------- the twin against torch autograd (fp64)
def _torch_loss(shape, sources, sym, data, critic_rows, obs_normalized, augment, mirror_coef):
    """The loss of include/upkie_hip.h, written out with torch ops in fp64; (stats without the norm, parameters)."""
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    asym = critic_rows is not None
    nf = AR.N_FIXED if asym else 4
    fixed = [t(s) for s in sources[:nf]]
    params = [t(s).clone().requires_grad_(True) for s in sources[nf:]]
    log_std = params[0]
    na = 2 * (int(shape.actor_layers) + 1)
    actor, critic = params[1:1 + na], params[1 + na:]
    act_fn = torch.tanh if int(shape.activation) == 0 else torch.relu

    def tower(layers, x):
        for i in range(0, len(layers), 2):
            x = x @ layers[i].T + layers[i + 1]
            if i + 2 < len(layers):
                x = act_fn(x)
        return x

    def normalise(x, mean, std):
        if obs_normalized or not int(shape.normalize):
            return x
        return ((x - mean) / std).clamp(-float(shape.clip_obs), float(shape.clip_obs))

    B = len(data["obs"])
    obs, actions = t(data["obs"]), t(data["actions"])
    xa = torch.cat([normalise(obs, fixed[0], fixed[1]), normalise(sym.mirror_obs(obs), fixed[0], fixed[1])])
    if asym:
        rows = t(critic_rows)
        xc = torch.cat([normalise(rows, fixed[4], fixed[5]), normalise(sym.mirror_critic_obs(rows), fixed[4], fixed[5])])
    else:
        xc = xa
    act = torch.cat([actions, sym.mirror_action(actions)])
    adv = t(data["advantages"])
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    adv, old_lp, old_v, ret = (torch.cat([v, v]) for v in (adv, t(data["log_probs"]), t(data["values"]), t(data["returns"])))
    keep = slice(0, 2 * B if augment else B)
    mu = tower(actor, xa)
    dist = torch.distributions.Normal(mu, torch.ones_like(mu) * log_std.exp())
    log_prob = dist.log_prob(act).sum(1)
    ratio = torch.exp(log_prob - old_lp)
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 0.8, 1.2))[keep].mean()
    v = tower(critic, xc).flatten()
    value_loss = torch.nn.functional.mse_loss(ret[keep], (old_v + torch.clamp(v - old_v, -0.2, 0.2))[keep])
    entropy_loss = -dist.entropy().sum(1).mean()
    mirror_loss = torch.nn.functional.mse_loss(mu[B:], sym.mirror_action(mu[:B]).detach())
    loss = policy_loss + CFG["ent_coef"] * entropy_loss + 0.5 * value_loss + mirror_coef * mirror_loss
    with torch.no_grad():
        log_ratio = (log_prob - old_lp)[:B]
        approx_kl = ((torch.exp(log_ratio) - 1.0) - log_ratio).mean()
        clip_fraction = ((ratio[:B] - 1.0).abs() > 0.2).double().mean()
    grads = torch.autograd.grad(loss, params)
    stats = [policy_loss, value_loss, entropy_loss, loss, approx_kl, clip_fraction, mirror_loss]
    return np.array([float(s.detach()) for s in stats]), [g.numpy() for g in grads]


def _symmetric_case(normalize):
    row = S.Row(37, 6, [24, 17], 3, [20], "tanh", "")
    shape = S.shape_of(row, normalize=normalize)
    sources = S.row_sources(row, *S.row_modules(row), normalize, log_std=SR.LOG_STD)
    sym = SR.row_mirror(row)
    data = SR.row_rollout(row, shape, sources, sym)
    return row, shape, sources, sym, data, None


def _asymmetric_case(normalize):
    row = AS.ROWS[0]
    shape = AS.shape_of(row, normalize=normalize)
    sources = AS.row_sources(row, *AS.row_modules(row), normalize, log_std=SR.LOG_STD)
    sym = SR.row_mirror(row, critic_dim=row.critic_obs_dim)
    data = AS.row_rollout(row, shape, sources)
    return row, shape, sources, sym, data, data["critic_observations"]


@pytest.mark.parametrize("case", [_symmetric_case, _asymmetric_case], ids=["symmetric", "asymmetric"])
@pytest.mark.parametrize("obs_normalized", [False, True])
@pytest.mark.parametrize("augment,mirror_coef", [(True, 0.0), (True, 0.7), (False, 0.7), (False, 0.0)])
def test_twin_against_torch_autograd(case, obs_normalized, augment, mirror_coef):
    row, shape, sources, sym, data, critic_rows = case(normalize=True)
    total = S.T * row.N
    flat = {"obs": data["observations"].reshape(total, -1), "actions": data["actions"].reshape(total, -1)}
    flat.update({k: data[k].reshape(total) for k in ("values", "log_probs", "advantages", "returns")})
    rows = None if critic_rows is None else critic_rows.reshape(total, -1)
    stats, grads, _, _ = SR.minibatch(shape, sources, sym, flat["obs"], flat["actions"], flat["values"], flat["log_probs"], flat["advantages"],
                                      flat["returns"], critic_obs=rows, obs_normalized=obs_normalized, augment=augment, mirror_coef=mirror_coef, **CFG)
    want_stats, want = _torch_loss(shape, sources, sym, flat, rows, obs_normalized, augment, mirror_coef)
    np.testing.assert_allclose(stats[[0, 1, 2, 3, 4, 5, 7]], want_stats, rtol=1e-12, atol=1e-12)
    assert len(grads) == len(want)
    for k, (g, w) in enumerate(zip(grads, want)):
        assert np.linalg.norm(g - w.reshape(g.shape)) <= 1e-12 * max(1.0, np.linalg.norm(w)), k
    assert abs(stats[6] - math.sqrt(sum(float(np.sum(g * g)) for g in grads))) <= 1e-12 * stats[6]


def test_both_switches_off_is_the_plain_twin():
    row, shape, sources, sym, data, _ = _symmetric_case(True)
    total = S.T * row.N
    args = [data[k].reshape(total, *data[k].shape[2:]) for k in ("observations", "actions", "values", "log_probs", "advantages", "returns")]
    stats, grads, ratio, _ = SR.minibatch(shape, sources, sym, *args, augment=False, mirror_coef=0.0, **CFG)
    plain_stats, plain_grads, plain_ratio = PR.minibatch(shape, sources, *args, **CFG)
    assert np.array_equal(stats[:7], plain_stats) and np.array_equal(ratio, plain_ratio)
    for g, p in zip(grads, plain_grads):
        assert np.array_equal(g, p)


# ---------------------------------------------------------------- the header against abi.py
def test_header_matches_abi(library):
    probe = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "upkie_hip.h"
    int main(void) {
      printf("%zu %zu %zu %zu %d %d %d\n", sizeof(UpkiePpoMirror), offsetof(UpkiePpoMirror, augment), offsetof(UpkiePpoMirror, mirror_coef),
             offsetof(UpkiePpoMirror, tables), UPKIE_PPO_MIRROR_STATS, UPKIE_STRUCT_PPO_MIRROR, UPKIE_STRUCT_COUNT);
      return 0;
    }
    """
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write(probe)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    m = abi.UpkiePpoMirror
    which = next(k for k, cls in abi.STRUCT_IDS.items() if cls is m)
    assert out == [C.sizeof(m), m.augment.offset, m.mirror_coef.offset, m.tables.offset, abi.PPO_MIRROR_STATS, which, len(abi.STRUCT_IDS)]
    assert len(MIRROR_STAT_NAMES) == abi.PPO_MIRROR_STATS == len(SR.STAT_NAMES) and MIRROR_STAT_NAMES == SR.STAT_NAMES
    assert library.upkie_hip_struct_bytes(which) == C.sizeof(m)
    for name in ("upkie_ppo_mirror_words", "upkie_ppo_mirror_set", "upkie_ppo_mirror_workspace_bytes", "upkie_ppo_minibatch_update_mirror"):
        assert name in lib.EXPORTED_SYMBOLS and getattr(library, name).argtypes is not None


# ---------------------------------------------------------------- refusals, by name
def _shape(D, widths, A, Dc=0):
    row = AS.Row(1, D, widths, A, Dc, widths, "tanh", "") if Dc else S.Row(1, D, widths, A, widths, "tanh", "")
    return AS.shape_of(row) if Dc else S.shape_of(row)


def test_mirror_symmetry_refuses_bad_tables_by_name():
    ok = dict(obs_index=[1, 0, 2], obs_sign=[1, 1, -1], act_index=[0, 1], act_sign=[1, -1])
    MirrorSymmetry(**ok)
    for change, match in (
        (dict(obs_index=[1, 2, 0]), "obs_index is not an involution"),
        (dict(act_index=[0, 2]), r"act_index\[1\] = 2 is out of range"),
        (dict(obs_index=[-1, 0, 2]), r"obs_index\[0\] = -1 is out of range"),
        (dict(obs_sign=[1, 1, 0]), r"obs_sign\[2\].*must be \+1 or -1"),
        (dict(act_sign=[1, 0.5]), r"act_sign\[1\].*must be \+1 or -1"),
        (dict(obs_sign=[1, -1, -1]), "obs_sign differs between the partners 0 and 1"),
        (dict(critic_index=[0, 1]), "critic_index and critic_sign come together"),
        (dict(critic_index=[1, 1], critic_sign=[1, 1]), "critic_index is not an involution"),
        (dict(mirror_coef=-0.1), "mirror_coef"),
        (dict(mirror_coef=math.nan), "mirror_coef"),
        (dict(mirror_coef=math.inf), "mirror_coef"),
    ):
        with pytest.raises(ValueError, match=match):
            MirrorSymmetry(**dict(ok, **change))


def _bare_policy(shape):
    pol = MlpActorCritic.__new__(MlpActorCritic)  # (the shape is all the checks read: no device needed)
    pol.shape = shape
    return pol


def test_trainer_refuses_by_name_before_any_device_use():
    sym = MirrorSymmetry.gyropod()
    with pytest.raises(ValueError, match="symmetry with a process_group is not supported"):
        PpoTrainer(_bare_policy(_shape(6, [16], 2)), symmetry=sym, process_group=object())
    with pytest.raises(ValueError, match="symmetry with a process_group is not supported"):
        Ppo.__init__(Ppo.__new__(Ppo), _FakeEnv(), _bare_policy(_shape(6, [16], 2)), symmetry=sym, process_group=object())
    with pytest.raises(TypeError, match="MirrorSymmetry"):
        PpoTrainer(_bare_policy(_shape(6, [16], 2)), symmetry=(GYROPOD_OBS_SIGN, GYROPOD_ACT_SIGN))
    with pytest.raises(ValueError, match="the mirror is of 6 observation and 2 action words, the policy takes 8 and 2"):
        PpoTrainer(_bare_policy(_shape(8, [16], 2)), symmetry=sym)
    with pytest.raises(ValueError, match="asymmetric.*needs critic_index and critic_sign"):
        PpoTrainer(_bare_policy(_shape(6, [16], 2, Dc=5)), symmetry=sym)
    with pytest.raises(ValueError, match="symmetric.*superfluous"):
        PpoTrainer(_bare_policy(_shape(6, [16], 2)), symmetry=MirrorSymmetry.signs(GYROPOD_OBS_SIGN, GYROPOD_ACT_SIGN, critic_sign=[1, -1]))
    with pytest.raises(ValueError, match="critic tables are of 2 words, the policy's critic takes 5"):
        PpoTrainer(_bare_policy(_shape(6, [16], 2, Dc=5)), symmetry=MirrorSymmetry.signs(GYROPOD_OBS_SIGN, GYROPOD_ACT_SIGN, critic_sign=[1, -1]))


class _FakeEnv:
    num_envs = 4
    device = "cpu"


def test_library_refuses_by_name_on_the_host(library):
    """upkie_ppo_mirror_set validates on the HOST, before any device use (the tables pointer here is not even device
    memory), and upkie_ppo_minibatch_update_mirror its coefficient."""
    err = lambda: library.upkie_sim_last_error(None)  # noqa: E731
    i32, f32 = lambda a: np.asarray(a, dtype=np.int32), lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    sym_shape, asym_shape = _shape(3, [16], 2), _shape(3, [16], 2, Dc=2)
    assert library.upkie_ppo_mirror_words(C.byref(sym_shape)) == 2 * (3 + 2)
    assert library.upkie_ppo_mirror_words(C.byref(asym_shape)) == 2 * (3 + 2 + 2)
    assert library.upkie_ppo_mirror_workspace_bytes(C.byref(sym_shape), 0) == abi.ERR_INVALID_ARGUMENT
    assert library.upkie_ppo_mirror_workspace_bytes(C.byref(sym_shape), 2**30) == abi.ERR_INVALID_ARGUMENT
    block = np.zeros(64, dtype=np.int32)

    def set_tables(shape, obs=([1, 0, 2], [1, 1, -1]), critic=None, act=([0, 1], [1, -1])):
        keep = [i32(obs[0]), f32(obs[1]), i32(act[0]), f32(act[1])] + ([] if critic is None else [i32(critic[0]), f32(critic[1])])
        p = [a.ctypes.data for a in keep]
        return library.upkie_ppo_mirror_set(C.byref(shape), p[0], p[1], p[4] if critic else None, p[5] if critic else None, p[2], p[3],
                                            block.ctypes.data, None)

    for kw, message in (
        (dict(obs=([1, 2, 0], [1, 1, 1])), b"obs_index is not an involution"),
        (dict(obs=([1, 0, 3], [1, 1, 1])), b"obs_index[2] = 3 is out of range"),
        (dict(act=([0, -1], [1, 1])), b"act_index[1] = -1 is out of range"),
        (dict(obs=([1, 0, 2], [1, 1, 0])), b"obs_sign[2] must be +1 or -1"),
        (dict(act=([0, 1], [1, math.nan])), b"act_sign[1] must be +1 or -1"),
        (dict(obs=([1, 0, 2], [1, -1, 1])), b"obs_sign differs between the partners 0 and 1"),
        (dict(critic=([1, 0], [1, 1])), b"critic tables are superfluous"),
    ):
        assert set_tables(sym_shape, **kw) == abi.ERR_INVALID_ARGUMENT and message in err(), (kw, err())
    assert set_tables(asym_shape) == abi.ERR_INVALID_ARGUMENT and b"needs critic_index and critic_sign" in err()
    assert set_tables(asym_shape, critic=([1, 1], [1, 1])) == abi.ERR_INVALID_ARGUMENT and b"critic_index is not an involution" in err()
    assert not block.any(), "nothing was written"
    if library.upkie_hip_device_count() == 0:
        assert set_tables(sym_shape) == abi.ERR_NO_DEVICE and set_tables(asym_shape, critic=([1, 0], [-1, -1])) == abi.ERR_NO_DEVICE

    cfg = abi.UpkiePpoConfig(0.2, 0.0, 0.0, 0.5, 0.5, 0.9, 0.999, 1e-5, 0, 0)
    buf = block.ctypes.data

    def update(coef, tables=buf, shape=sym_shape, size=32, control=None):
        mirror = abi.UpkiePpoMirror(1, coef, tables)
        return library.upkie_ppo_minibatch_update_mirror(C.byref(shape), C.byref(cfg), C.byref(mirror), 64, 0, size, 32, buf, buf, None, buf, buf, buf,
                                                         buf, buf, buf, buf, buf, buf, buf, control, buf, buf, None)

    for coef in (-0.5, math.nan, math.inf):
        assert update(coef) == abi.ERR_INVALID_ARGUMENT and b"mirror_coef must be finite and not negative" in err()
    assert update(0.5, tables=None) == abi.ERR_INVALID_ARGUMENT and b"null mirror" in err()
    assert update(0.5, size=33) == abi.ERR_INVALID_ARGUMENT and b"minibatch" in err()
    assert update(0.5, shape=asym_shape) == abi.ERR_INVALID_ARGUMENT and b"asymmetric" in err()
    assert update(0.5, control=buf + 4) == abi.ERR_INVALID_ARGUMENT and b"aligned" in err()
    if library.upkie_hip_device_count() == 0:
        assert update(0.5) == abi.ERR_NO_DEVICE


# ---------------------------------------------------------------- the builders
def test_builders():
    g = MirrorSymmetry.gyropod(("ground_velocity", "yaw_velocity"), mirror_coef=0.5)
    assert g.obs_sign.tolist() == [1, 1, -1, 1, 1, -1, 1, -1] and g.obs_index.tolist() == list(range(8))
    assert g.act_sign.tolist() == [1, -1] and g.mirror_coef == 0.5 and g.augment

    class Pipeline:
        obs_dim, act_dim, stack, action_in_observation = 8, 2, 3, True

    p = g.for_pipeline(Pipeline)
    assert p.obs_sign.tolist() == ([1, 1, -1, 1, 1, -1, 1, -1] + [1, -1]) * 3 and p.obs_index.tolist() == list(range(30))
    assert p.mirror_coef == 0.5
    Pipeline.action_in_observation = False
    assert g.for_pipeline(Pipeline).obs_sign.size == 24
    swap = MirrorSymmetry([1, 0], [1, 1], [1, 0], [-1, -1])
    Pipeline.obs_dim, Pipeline.action_in_observation, Pipeline.stack = 2, True, 2
    assert swap.for_pipeline(Pipeline).obs_index.tolist() == [1, 0, 3, 2, 5, 4, 7, 6]
    x = np.arange(8.0)
    assert np.array_equal(g.mirror_obs(g.mirror_obs(x)), x) and np.array_equal(swap.mirror_action(np.array([1.0, 2.0])), [-2.0, -1.0])
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 6, 64, 255):
        index, sign = SR.signed_involution(n, rng)
        assert (index[index] == np.arange(n)).all() and (sign[index] == sign).all() and (sign < 0).any()
        assert n < 2 or 0.3 * n <= (index != np.arange(n)).sum() <= 0.7 * n + 1, "about half the words are swapped"


# ---------------------------------------------------------------- the Gyropod table against the fp64 oracle
def test_gyropod_table_is_the_oracles_mirror():
    """Two copies of one env, one driven with (v, w) and one with (v, -w), through a fall: under the table's signs the
    observations agree to 1e-7 (measured: 4.4e-9, the fall at step 136). The drive is smooth from rest on purpose: the
    oracle's contact solver stops at a tolerance, its residual is not mirror-symmetric, and a command that jumps leaves one
    of 1e-5 (a step to (1.0, 0.5) at rest: 4.7e-5 by step 6), which says nothing about the table."""
    from oracle import oracle as O
    from upkie_amd.model.default_model import default_model

    def make():
        o = O.Oracle(default_model(), abi.default_sim_config(num_envs=1, seed=3))
        return o, o.reset()

    (a, obs_a), (b, obs_b) = make(), make()
    sign = np.array(GYROPOD_OBS_SIGN)
    assert np.array_equal(obs_a, obs_b)
    worst, fell, yaw = 0.0, None, 0.0
    for k in range(400):
        act = np.array([[0.004 * k, 0.5 * math.sin(0.02 * k)]])  # (smooth from rest: see the docstring)
        obs_a, _, term_a, _ = a.step_gyropod(act)
        obs_b, _, term_b, _ = b.step_gyropod(act * np.array(GYROPOD_ACT_SIGN))
        worst = max(worst, float(np.abs(obs_b - sign * obs_a).max()))
        yaw = max(yaw, float(np.abs(obs_a[0, [2, 5]]).max()))
        assert term_a[0] == term_b[0]
        if term_a[0]:
            fell = k
            break
    print(f"\nsymmetry gyropod fell_at={fell} worst={worst:.3e} max_yaw_word={yaw:.3e}")
    assert fell is not None and fell >= 130, "130+ steps, through a fall"
    assert yaw > 0.1, "the flipped words moved"
    assert worst <= 1e-7


# ---------------------------------------------------------------- the input conditions of the GPU tests
def _row_inputs(index, row):
    shape = S.shape_of(row, normalize=S.row_normalize(index))
    sources = SR.row_sources(index, row)
    sym, data = SR.conditioned_inputs(row, shape, sources)
    assert SR.condition(shape, sources, sym, data) <= SR.MAX_CONDITION
    total = S.T * row.N
    args = [data[k].reshape(total, *data[k].shape[2:]) for k in ("observations", "actions", "values", "log_probs", "advantages", "returns")]
    return shape, sources, sym, args


@pytest.fixture(scope="module")
def row_twins():
    """The twin of every MATRIX row on the GPU tests' inputs, computed once."""
    out = []
    for index, row in enumerate(S.MATRIX):
        shape, sources, sym, args = _row_inputs(index, row)
        out.append((shape, sources, sym, args, SR.minibatch(shape, sources, sym, *args, augment=True, mirror_coef=COEF, **CFG)))
    return out


@pytest.mark.parametrize("index", range(len(S.MATRIX)), ids=[S.row_id(r) for r in S.MATRIX])
def test_gpu_input_conditions(index, row_twins):
    row = S.MATRIX[index]
    shape, sources, sym, args, (stats, grads, ratio, ratio_m) = row_twins[index]
    total = S.T * row.N
    assert (sym.obs_sign < 0).any() and (sym.act_sign < 0).any()
    assert row.obs_dim < 2 or (sym.obs_index != np.arange(row.obs_dim)).any()
    for r in (ratio, ratio_m):
        for edge in (0.8, 1.2):
            assert not (np.abs(r - edge) < 1e-3).any(), "no original or mirrored ratio within 1e-3 of a clip bound"
    worst = float(np.abs(np.log(ratio_m)).max())
    regimes = [float(np.mean(ratio_m < 0.8)), float(np.mean((ratio_m >= 0.8) & (ratio_m <= 1.2))), float(np.mean(ratio_m > 1.2))]
    print(f"\nsymmetry inputs {S.row_id(row)} worst_log_ratio={worst:.2f} below={regimes[0]:.3f} inside={regimes[1]:.3f} above={regimes[2]:.3f} "
          f"mirror_loss={stats[7]:.3e}")
    assert worst <= 8.0
    if total >= 30:
        assert min(regimes) >= 0.05, regimes
    assert stats[7] > 1e-4, "the policy is not symmetric under the mirror: the mirror loss has something to say"


@pytest.mark.parametrize("mutation", SR.MUTATIONS)
def test_gpu_inputs_tell_the_mistakes_from_the_feature(mutation, row_twins):
    """Every one-line mistake moves some gradient tensor (or, for the KL's denominator, approx_kl) by at least 100 of the
    GPU test's bounds, on every row where it changes anything at all."""
    for index, row in enumerate(S.MATRIX):
        if mutation == "normalise_before_mirror" and not S.row_normalize(index):
            continue  # (without normalisation there is nothing to order)
        shape, sources, sym, args, (stats, grads, _, _) = row_twins[index]
        wrong_stats, wrong, _, _ = SR.minibatch(shape, sources, sym, *args, augment=True, mirror_coef=COEF, mutation=mutation, **CFG)
        if mutation == "kl_over_n":
            # (no gradient word depends on it. Measured as the gradient is, relatively: 100 gradient bounds of approx_kl;
            # and in the GPU test's own terms: ten times the 1e-5 it holds approx_kl to)
            moved = abs(wrong_stats[4] - stats[4])
            print(f"\nsymmetry kl_over_n {S.row_id(row)} moved={moved:.3e} approx_kl={stats[4]:.3e}")
            assert moved >= 100 * S.bounds(row)["grad"] * stats[4] and moved >= 10 * 1e-5, (S.row_id(row), wrong_stats[4], stats[4])
            continue
        moved = max(np.linalg.norm(w - g) / max(np.linalg.norm(g), 1e-30) for w, g in zip(wrong, grads))
        assert moved >= 100 * S.bounds(row)["grad"], (S.row_id(row), mutation, moved)
