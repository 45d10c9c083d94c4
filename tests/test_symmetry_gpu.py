"""The mirrored PPO update (upkie_ppo_minibatch_update_mirror, csrc/ppo.hpp MIR = true) on the MI355X against the fp64
twin of tests/symmetry_reference.py: the gradient launch on every row of tests/mlp_shapes.MATRIX (all ten instantiations,
blocks of 1 to 4 waves, dot and MFMA heads, 64 actions over four tiles, 255- and 256-word rows) on the inputs whose
conditions tests/test_symmetry.py asserts, the edge minibatches, an asymmetric row, each switch alone, identity tables, a
full update, determinism and graph replay, the workspace and the words the update must not write, target_kl on the
originals' KL, and `Ppo(symmetry=)` on a Gyropod env.

Each gradient test prints `symmetry <family> <id> <figure>=<value> ...` before it asserts."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import asymmetric_reference as AR
from tests import asymmetric_shapes as AS
from tests import mlp_shapes as S
from tests import ppo_reference as PR
from tests import symmetry_reference as SR
from tests.training_rig import same, snapshot, tower, warm_up_as_the_capture_does
from upkie_amd import abi
from upkie_amd.ppo import MIRROR_STAT_NAMES, Ppo, PpoTrainer, trainable_offset
from upkie_amd.rollout import RolloutBuffer
from upkie_amd.symmetry import MirrorSymmetry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = S.DEV
BETA1_F32 = np.float32(1.0) - np.float32(0.9)
CFG = dict(ent_coef=0.01, clip_range_vf=0.2, max_grad_norm=1e9)
COEF = 0.5
KEYS = ("observations", "actions", "values", "log_probs", "advantages", "returns")
MAX_GRID = 512  # PPO_MAX_GRID


def _np(t):
    return t.detach().double().cpu().numpy()


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _flat(data, B):
    """The first B samples of a rollout's arrays, flattened over (T, N)."""
    out = {k: data[k].reshape(-1, *data[k].shape[2:])[:B] for k in KEYS}
    if "critic_observations" in data:
        out["critic_observations"] = data["critic_observations"].reshape(-1, data["critic_observations"].shape[-1])[:B]
    return out


def _buffer(flat, B):
    """A full one-step buffer of the B samples."""
    D, A = flat["observations"].shape[-1], flat["actions"].shape[-1]
    rows = flat.get("critic_observations")
    buf = RolloutBuffer(1, B, obs_shape=(D,), action_shape=(A,), device=DEV, critic_obs_shape=None if rows is None else (rows.shape[-1],))
    for name in ("observations", "actions", "values", "log_probs") + (("critic_observations",) if rows is not None else ()):
        getattr(buf, name).copy_(torch.as_tensor(flat[name], device=DEV).reshape(getattr(buf, name).shape))
    buf.advantages = torch.as_tensor(flat["advantages"], device=DEV).reshape(1, B)
    buf.returns = torch.as_tensor(flat["returns"], device=DEV).reshape(1, B)
    buf.pos, buf.full = 1, True
    return buf


def _one_minibatch(pol, sym, flat, B, **kw):
    """One minibatch of all B samples from a fresh optimiser state, no norm clip: (trainer, the gradient per trainable
    tensor read back from Adam's first moment, the statistics row, the permutation)."""
    buf = _buffer(flat, B)
    tr = PpoTrainer(pol, n_epochs=1, batch_size=B, seed=3, symmetry=sym, **dict(CFG, **kw))
    tr.prepare(buf)
    stats = tr.update(buf, sync=False)
    torch.cuda.synchronize()
    grads = [_np(m) / float(BETA1_F32) for m in tr.state_dict()["m"]]
    return tr, grads, stats.double().cpu().numpy()[0, 0], tr.perm[0].long().cpu().numpy()


def _twin(shape, src0, sym, flat, idx, **kw):
    args = [flat[k].astype(np.float64)[idx] for k in KEYS]
    rows = flat.get("critic_observations")
    return SR.minibatch(shape, src0, sym, *args, critic_obs=None if rows is None else rows.astype(np.float64)[idx], **dict(CFG, **kw))


def _hold(family, name, grads, stats, ref_grads, ref_stats, bound, B, **figures):
    """The relative Frobenius error of every gradient tensor at `bound`, the statistics as tests/test_ppo_gpu.py holds
    them (mirror_loss like a loss)."""
    errors = [_rel(g.reshape(r.shape), r) for g, r in zip(grads, ref_grads)]
    worst = int(np.argmax(errors))
    print(f"\nsymmetry {family} {name} B={B} worst_tensor={worst} grad={errors[worst]:.3e} bound_grad={bound:.1e} kl={abs(stats[4] - ref_stats[4]):.2e} "
          f"mirror_loss={stats[7]:.6e} twin_mirror_loss={ref_stats[7]:.6e} " + " ".join(f"{k}={v}" for k, v in figures.items()))
    assert len(grads) == len(ref_grads)
    for k, e in enumerate(errors):
        assert e <= bound, (k, e)
    np.testing.assert_allclose(stats[[0, 1, 2, 3, 6, 7]], ref_stats[[0, 1, 2, 3, 6, 7]], rtol=1e-4, atol=1e-6)
    assert abs(stats[4] - ref_stats[4]) <= 1e-5 and abs(stats[5] - ref_stats[5]) <= 1.0 / B


def _matrix_policy(index, row):
    log_std = nn.Parameter(torch.full((row.act_dim,), SR.LOG_STD, device=DEV))
    pol, _, _, _ = S.policy(row.obs_dim, row.actor, row.act_dim, row.activation, seed=row.seed, normalize=S.row_normalize(index),
                            critic_widths=row.critic, log_std=log_std)
    return pol


ROWS = [pytest.param(i, r, id=f"W{S.width_class(S.shape_of(r))}-{r.activation}-nw{PR.plan(S.shape_of(r))['nw']}-{S.row_id(r)}")
        for i, r in enumerate(S.MATRIX)]


# ---------------------------------------------------------------- the gradient launch on every row of the matrix
@pytest.mark.parametrize("index,row", ROWS)
def test_gradient_against_the_fp64_twin(index, row):
    pol = _matrix_policy(index, row)
    src0 = S.sources_of(pol)
    for k, (a, b) in enumerate(zip(SR.row_sources(index, row), src0)):  # (the inputs tests/test_symmetry.py checked)
        assert np.array_equal(np.asarray(a).reshape(-1), b.reshape(-1)), k
    sym, data = SR.conditioned_inputs(row, pol.shape, src0, augment=True, mirror_coef=COEF)
    B = S.T * row.N
    flat = _flat(data, B)
    tr, grads, stats, idx = _one_minibatch(pol, sym, flat, B)
    ref_stats, ref_grads, _, _ = _twin(pol.shape, src0, sym, flat, idx, augment=True, mirror_coef=COEF)
    plan = PR.plan(pol.shape)
    _hold("gradient", S.row_id(row), grads, stats, ref_grads, ref_stats, S.bounds(row)["grad"], B, nw=plan["nw"], chunks=PR.chunks(plan, 2 * B),
          grid_cap=plan["grid_cap"])


EDGE = S.Row(8200, 6, [64, 64], 2, [64, 64], "relu", "four-wave blocks; two actions on an MFMA head")


@pytest.mark.parametrize("B", [1, 8, 9, 40, 16400])
def test_edge_minibatches(B):
    """One sample (one pair); 8 (exactly one tile of pairs); 9 (a second tile with one pair); 40 (80 positions: the last
    chunk of four-wave blocks has one tile, three waves idle); 16400 (257 chunks of plain tiles, under PPO_MAX_GRID; 513 of
    doubled ones, over it: blocks take a second chunk and add to their partials)."""
    row = EDGE
    plan = PR.plan(S.shape_of(row))
    assert plan["nw"] == 4 and plan["grid_cap"] == MAX_GRID
    if B == 16400:
        assert PR.chunks(plan, B) < MAX_GRID < PR.chunks(plan, 2 * B)
    if B == 40:
        assert PR.chunks(plan, 2 * B) == 2 and (2 * B + 15) // 16 == 5
    pol = _matrix_policy(1, row)
    src0 = S.sources_of(pol)
    sym, data = SR.conditioned_inputs(row, pol.shape, src0, samples=B, augment=True, mirror_coef=COEF)
    flat = _flat(data, B)
    tr, grads, stats, idx = _one_minibatch(pol, sym, flat, B)
    ref_stats, ref_grads, _, _ = _twin(pol.shape, src0, sym, flat, idx, augment=True, mirror_coef=COEF)
    _hold("edge", S.row_id(row), grads, stats, ref_grads, ref_stats, S.DEFAULT_BOUNDS["grad"], B)


@pytest.mark.parametrize("index", [1, 5], ids=[AS.row_id(AS.ROWS[1]), AS.row_id(AS.ROWS[5])])
@pytest.mark.parametrize("obs_normalized", [False, True])
def test_asymmetric_row_with_critic_tables(index, obs_normalized):
    row = AS.ROWS[index]
    log_std = nn.Parameter(torch.full((row.act_dim,), SR.LOG_STD, device=DEV))
    pol, _, _, _ = AS.policy(row, normalize=True, log_std=log_std)
    src0 = S.sources_of(pol)
    sym, data = SR.conditioned_inputs(row, pol.shape, src0, rollout=SR.asymmetric_row_rollout, critic_dim=row.critic_obs_dim, augment=True,
                                      mirror_coef=COEF)
    B = S.T * row.N
    flat = _flat(data, B)
    if obs_normalized:  # (the stored rows are mirrored as they are: keep them where the networks are used to)
        flat["observations"], flat["critic_observations"] = flat["observations"].clip(-3, 3), flat["critic_observations"].clip(-3, 3)
        flat = _flat(SR._nudge({k: v[None] for k, v in flat.items()}, *_log_probs(pol.shape, src0, sym, flat)), B)
    tr, grads, stats, idx = _one_minibatch(pol, sym, flat, B, obs_normalized=obs_normalized)
    ref_stats, ref_grads, _, _ = _twin(pol.shape, src0, sym, flat, idx, augment=True, mirror_coef=COEF, obs_normalized=obs_normalized)
    _hold("asymmetric", AS.row_id(row), grads, stats, ref_grads, ref_stats, AS.BOUNDS["grad"], B, obs_normalized=obs_normalized)


def _log_probs(shape, src0, sym, flat):
    """(log-prob of the stored actions, of the mirrored ones on the mirrored rows) when the rows are stored normalised."""
    from tests import mlp_reference as R

    raw = abi.UpkieMlpShape.from_buffer_copy(shape)
    raw.normalize = 0
    obs, rows, act = (flat[k].astype(np.float64) for k in ("observations", "critic_observations", "actions"))
    log_std = np.asarray(src0[AR.N_FIXED], dtype=np.float64)
    _, mean, _, _ = AR.forward(raw, src0, obs, rows)
    _, mean_m, _, _ = AR.forward(raw, src0, sym.mirror_obs(obs), rows)
    return R.log_prob(act, mean, log_std), R.log_prob(sym.mirror_action(act), mean_m, log_std)


# ---------------------------------------------------------------- each switch alone, both off, identity tables
SWITCH_ROWS = (4, 16)  # 1001-5-[40,24]-3 tanh (widths off the tiles); 33-6-[32]-64 relu (four action tiles)


@pytest.mark.parametrize("index", SWITCH_ROWS)
def test_mirror_loss_alone(index):
    """augment off, mirror_coef > 0: the partners carry the mirror loss's dZ and nothing else; the means run over B."""
    row = S.MATRIX[index]
    pol = _matrix_policy(index, row)
    src0 = S.sources_of(pol)
    sym = SR.row_mirror(row, augment=False, mirror_coef=COEF)
    B = S.T * row.N
    flat = _flat(SR.row_rollout(row, pol.shape, src0, sym), B)
    tr, grads, stats, idx = _one_minibatch(pol, sym, flat, B)
    ref_stats, ref_grads, _, _ = _twin(pol.shape, src0, sym, flat, idx, augment=False, mirror_coef=COEF)
    _hold("mirror_loss_alone", S.row_id(row), grads, stats, ref_grads, ref_stats, S.bounds(row)["grad"], B)


@pytest.mark.parametrize("index", SWITCH_ROWS)
def test_both_switches_off_is_the_plain_gradient(index):
    row = S.MATRIX[index]
    pol = _matrix_policy(index, row)
    src0 = S.sources_of(pol)
    sym = SR.row_mirror(row, augment=False, mirror_coef=0.0)
    B = S.T * row.N
    flat = _flat(SR.row_rollout(row, pol.shape, src0, sym), B)
    tr, grads, stats, idx = _one_minibatch(pol, sym, flat, B)
    plain_stats, plain_grads, _ = PR.minibatch(pol.shape, src0, *[flat[k].astype(np.float64)[idx] for k in KEYS], **CFG)
    ref_stats, _, _, _ = _twin(pol.shape, src0, sym, flat, idx, augment=False, mirror_coef=0.0)
    assert np.array_equal(ref_stats[:7], plain_stats)
    _hold("both_off", S.row_id(row), grads, stats, plain_grads, ref_stats, S.bounds(row)["grad"], B)


@pytest.mark.parametrize("index", SWITCH_ROWS + (0,))
def test_identity_tables(index):
    """The identity mirror: every partner is its original, so mirror_loss is 0.0 exactly (the partner's lane computes the
    original's mean bit for bit) and the augmented gradient is the plain one."""
    row = S.MATRIX[index]
    pol = _matrix_policy(index, row)
    src0 = S.sources_of(pol)
    sym = SR.identity_mirror(row, augment=True, mirror_coef=COEF)
    B = S.T * row.N
    flat = _flat(S.row_rollout(row, pol.shape, src0), B)
    tr, grads, stats, idx = _one_minibatch(pol, sym, flat, B)
    assert stats[7] == 0.0, stats[7]
    plain_stats, plain_grads, _ = PR.minibatch(pol.shape, src0, *[flat[k].astype(np.float64)[idx] for k in KEYS], **CFG)
    _hold("identity", S.row_id(row), grads, stats, plain_grads, np.append(plain_stats, 0.0), S.bounds(row)["grad"], B)


# ---------------------------------------------------------------- a full update, bits, the words it must not write
def _trainer_case(index=4, **kw):
    row = S.MATRIX[index]
    pol = _matrix_policy(index, row)
    src0 = S.sources_of(pol)
    sym, data = SR.conditioned_inputs(row, pol.shape, src0, augment=True, mirror_coef=COEF)
    total = S.T * row.N
    flat = _flat(data, total)
    buf = _buffer(flat, total)
    return row, pol, src0, sym, flat, buf, total


def test_one_full_update_against_the_fp64_twin():
    """2 epochs x 3 minibatches, the last one short, clip and Adam: the parameters under tests/test_ppo_gpu.py's step bound,
    summed over the six steps."""
    row, pol, src0, sym, flat, buf, total = _trainer_case()
    lr, batch = 1e-3, (total + 2) // 3 + 1
    assert total % batch != 0 and (total + batch - 1) // batch == 3
    tr = PpoTrainer(pol, lr=lr, n_epochs=2, batch_size=batch, seed=5, symmetry=sym, ent_coef=0.01, clip_range_vf=0.2)
    fixed = trainable_offset(pol.shape)
    packed0, tables0 = pol.packed.clone(), tr.mirror_tables.clone()
    stats = tr.train(buf).double().cpu().numpy()
    torch.cuda.synchronize()
    assert stats.shape == (2, 3, 8)
    sources = [np.array(s) for s in src0]
    params = PR.trainable(pol.shape, sources)
    m, v, t = [0 * p for p in params], [0 * p for p in params], 0
    bound = [np.zeros_like(p) for p in params]
    for e in range(2):
        perm = tr.perm[e].long().cpu().numpy()
        for j in range(3):
            idx = perm[j * batch:(j + 1) * batch]
            ref_stats, grads, _, _ = _twin(pol.shape, sources, sym, flat, idx, augment=True, mirror_coef=COEF, max_grad_norm=0.5)
            np.testing.assert_allclose(stats[e, j][[0, 1, 2, 3, 6, 7]], ref_stats[[0, 1, 2, 3, 6, 7]], rtol=1e-3, atol=1e-5)
            coef = min(1.0, 0.5 / (ref_stats[6] + 1e-6))
            for k, g in enumerate(grads):  # (tests/test_ppo_gpu.py's bound of one step, for this step's gradient)
                delta = 1e-5 * np.linalg.norm(g) * coef + 1e-6 * np.abs(g) * coef
                bound[k] += lr * delta / (np.abs(g) * coef + 1e-5) + 2e-7 * np.abs(params[k]) + 1e-9
            params, m, v, t = PR.adam_step(params, grads, m, v, t, 0.5, lr)
            sources = sources[:4] + list(params)
    assert tr.state_dict()["t"] == 6
    after = [_np(p) for p in pol.sources()[4:]]
    for k, (p1, pr) in enumerate(zip(after, params)):
        assert np.all(np.abs(p1.reshape(pr.shape) - pr) <= bound[k]), (k, np.max(np.abs(p1.reshape(pr.shape) - pr) / bound[k]))
    assert torch.equal(pol.packed[:fixed], packed0[:fixed]), "the fixed words are never written"
    assert torch.equal(tr.mirror_tables, tables0), "the table block is never written"


def _state(pol, tr):
    return [pol.packed.clone(), tr.m.clone(), tr.v.clone(), tr.control.clone()]


def _restore(pol, tr, st):
    for dst, src in zip((pol.packed, tr.m, tr.v, tr.control), st):
        dst.copy_(src)


@pytest.mark.parametrize("index", [4, 2])
def test_deterministic_graph_replay_and_a_workspace_of_nan_bits(index):
    """Two updates from the same state give the same bits; so does a captured one; so does one whose workspace holds NaN
    bits behind its header (every partial word is written before it is added to or read)."""
    row, pol, src0, sym, flat, buf, total = _trainer_case(index)
    tr = PpoTrainer(pol, n_epochs=2, batch_size=(total + 2) // 3, seed=1, ent_coef=0.003, symmetry=sym)
    tr.prepare(buf)
    s0 = _state(pol, tr)
    runs = []
    for fill in (False, True):
        _restore(pol, tr, s0)
        if fill:
            tr.workspace[256:].view(torch.int32).fill_(0x7FC00000)
        stats = tr.update(buf, sync=False).clone()
        torch.cuda.synchronize()
        runs.append(_state(pol, tr) + [stats])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], s0[0]) and not torch.isnan(runs[0][4]).any()
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


def test_target_kl_reads_the_originals_alone():
    """A deliberately asymmetric policy on a first update (every original's ratio is 1, the partners' far from it): approx_kl
    is 0 and a small target_kl does NOT stop at minibatch 0; once the weights have moved a later minibatch stops, and from
    then on all 8 words are NaN."""
    row = S.MATRIX[4]
    pol = _matrix_policy(4, row)
    src0 = S.sources_of(pol)
    sym = SR.row_mirror(row, augment=True, mirror_coef=COEF)
    total = S.T * row.N
    flat = _flat(SR.row_rollout(row, pol.shape, src0, sym), total)
    from tests import mlp_reference as R

    _, mean, _ = R.forward(pol.shape, src0, flat["observations"].astype(np.float64))
    log_std = np.asarray(src0[4], dtype=np.float64)
    flat["log_probs"] = R.log_prob(flat["actions"].astype(np.float64), mean, log_std).astype(np.float32)  # (ratio 1)
    buf = _buffer(flat, total)
    tr = PpoTrainer(pol, lr=1e-2, n_epochs=4, batch_size=total // 4, seed=2, symmetry=sym, target_kl=1e-3)
    stats = tr.train(buf).double().cpu().numpy().reshape(-1, 8)
    _, _, _, ratio_m = _twin(pol.shape, src0, sym, flat, np.arange(total), augment=True, mirror_coef=COEF)
    partners_kl = float(np.mean((ratio_m - 1.0) - np.log(ratio_m)))
    ran = ~np.isnan(stats).any(axis=1)
    print(f"\nsymmetry target_kl partners_kl={partners_kl:.3e} first_kl={stats[0, 4]:.3e} ran={int(ran.sum())} of {len(ran)}")
    assert partners_kl > 1.5e-3 * 10, "the partners' KL alone would have stopped minibatch 0"
    assert ran[0] and abs(stats[0, 4]) <= 1e-6 and ran.sum() >= 2, "the first minibatch ran and stepped"
    stopped = int(ran.sum())
    assert stopped < len(ran), "a later minibatch stopped the update"
    assert stats[stopped - 1, 4] > 1.5e-3 and np.isnan(stats[stopped:]).all(), "8 NaN words from the stop on"
    assert tr.log()["early_stopped_at"] == divmod(stopped - 1, tr.n_minibatches) and "mirror_loss" in tr.log()
    assert float(tr.control[abi.PPO_CTRL_T]) == stopped - 1


# ---------------------------------------------------------------- Ppo(symmetry=) on a Gyropod env
def _gyropod(B=32, **kw):
    import upkie_amd.envs as envs
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    env = envs.make("Upkie-HIP-Gyropod-Vec", num_envs=B, frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=40)
    dev = env.device
    actor, critic = tower(6, 2).to(dev), tower(6, 1).to(dev)
    policy = MlpActorCritic.from_modules(actor, critic, nn.Parameter(torch.zeros(2, device=dev)), action_low=[-1.0, -1.0], action_high=[1.0, 1.0], seed=0)
    args = dict(n_steps=8, n_epochs=2, batch_size=64, seed=0, symmetry=MirrorSymmetry.gyropod(mirror_coef=1.0))
    return env, policy, dict(args, **kw)


def test_ppo_graphed_equals_eager_and_resumes_bit_for_bit(tmp_path):
    per, ends = 32 * 8, []
    for graph in (True, False):
        env, policy, kw = _gyropod(graph=graph)
        with env:
            model = Ppo(env, policy, **kw)
            if not graph:
                warm_up_as_the_capture_does(model)
            model.learn(4 * per)
            ends.append(snapshot(model))
    assert same(ends[0], ends[1]), "the graphed run equals the eager one, bit for bit"
    records = ends[0][1]
    assert len(records) == 4 and all(r["train/mirror_loss"] > 0.0 for r in records)
    assert set(f"train/{n}" for n in MIRROR_STAT_NAMES) <= set(records[0])
    path = str(tmp_path / "ppo.pt")
    env, policy, kw = _gyropod()
    with env:
        first = Ppo(env, policy, **kw).learn(4 * per, callback=lambda m, rec: m.iterations < 2)
        assert first.iterations == 2
        first.save(path)
    env, policy, kw = _gyropod()
    with env:
        resumed = Ppo.load(path, env, policy, **kw)  # (symmetry is code: given again)
        resumed.learn(2 * per, reset_num_timesteps=False)
        state, resumed_records = snapshot(resumed)
    assert same(state, ends[0][0]), "2 + save + load + 2 iterations equal 4 iterations, bit for bit"
    assert same(resumed_records, records[2:])


def test_fifty_updates_follow_the_twins_mirror_loss_curve():
    """50 full-batch updates with mirror_coef = 1 on one Gyropod rollout, against 50 fp64 updates from the same weights on
    the same (normalised) rows. mirror_loss is held like a loss (1e-4) at the first update and at 1e-3 along the curve:
    fp32 gradient words at rounding level take Adam steps of their own (up to lr each), which moves the loss by their
    gradient times that, second order."""
    env, policy, kw = _gyropod(n_epochs=50, batch_size=256, learning_rate=1e-3, graph=False)
    with env:
        src0 = S.sources_of(policy)
        model = Ppo(env, policy, **kw).learn(256)
        torch.cuda.synchronize()
        tr, buf, sym = model.trainer, model.buffer, kw["symmetry"]
        curve = tr.stats.double().cpu().numpy()[:, 0, 7]
        flat = {k: _np(getattr(buf, k)).reshape(256, -1) if k in ("observations", "actions") else _np(getattr(buf, k)).reshape(256)
                for k in ("observations", "actions", "values", "log_probs")}
        flat["advantages"], flat["returns"] = _np(tr.advantages), _np(tr.returns)
        perms = tr.perm.long().cpu().numpy()
        shape = policy.shape
    sources = [np.array(s) for s in src0]
    sources[0], sources[1] = np.zeros(6), np.ones(6)  # (the rows are stored normalised: obs_normalized)
    params = PR.trainable(shape, sources)
    m, v, t, twin = [0 * p for p in params], [0 * p for p in params], 0, []
    for e in range(50):
        ref_stats, grads, _, _ = _twin(shape, sources, sym, flat, perms[e], augment=True, mirror_coef=1.0, obs_normalized=True, ent_coef=0.0,
                                       clip_range_vf=None, max_grad_norm=0.5)
        twin.append(ref_stats[7])
        params, m, v, t = PR.adam_step(params, grads, m, v, t, 0.5, 1e-3)
        sources = sources[:4] + list(params)
    twin = np.array(twin)
    print(f"\nsymmetry curve first={curve[0]:.6e} twin_first={twin[0]:.6e} last={curve[-1]:.6e} twin_last={twin[-1]:.6e} "
          f"worst_rel={np.max(np.abs(curve - twin) / twin):.3e}")
    assert abs(twin[-1] - twin[0]) > 100 * 1e-3 * twin[0], "the curve moves by far more than it is held to: following it says something"
    np.testing.assert_allclose(curve[0], twin[0], rtol=1e-4)
    np.testing.assert_allclose(curve, twin, rtol=1e-3)


def test_example_runs():
    env = dict(os.environ, EXAMPLE_ENVS="64", EXAMPLE_STEPS="16", EXAMPLE_ITERATIONS="2")
    result = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_learn_symmetry.py")], capture_output=True, text=True, timeout=600,
                            env=env, cwd=os.path.join(ROOT, "examples"))
    assert result.returncode == 0, result.stderr[-3000:]
    lines = [ln for ln in result.stdout.splitlines() if ln.startswith("iteration")]
    assert len(lines) == 2 and all("train/mirror_loss" in ln and "nan" not in ln.split(",")[0] for ln in lines), result.stdout
