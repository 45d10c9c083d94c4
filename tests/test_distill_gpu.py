"""Policy distillation on the MI355X: the gradient launch against the fp64 twin of tests/distill_reference.py on every row
of tests/mlp_shapes.py's MATRIX, one full update, the words that get no gradient, determinism and graph replay, the mix
against its twin bit for bit, and the `Distillation` driver: graphed against eager, save / load, what it stores, an
`EvalCallback`, beta's ends, a fit against the twin's loss curve, the example.

The gradient tests print a line `distill <family> <id> <figure>=<value> ...` before they assert:
profiles/distill_matrix.txt is that output."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import asymmetric_shapes as AS
from tests import distill_reference as R
from tests import mlp_shapes as S
from tests import ppo_reference as PR
from tests.training_rig import bits, np64, pendulum, rel, same, snapshot, tower, warm_up_as_the_capture_does
from upkie_amd import abi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = S.DEV
T = S.T
BETA1_F32 = np.float32(1.0) - np.float32(0.9)
GRAD_BOUND = S.DEFAULT_BOUNDS["grad"]


def _param(index, row):
    plan = R.actor_plan(S.shape_of(row))
    return pytest.param(index, row, id=f"W{S.width_class(S.shape_of(row))}-{row.activation}-nw{plan['nw']}-{S.row_id(row)}")


ROWS = [_param(i, r) for i, r in enumerate(S.MATRIX)]


def _student(index, row):
    pol, actor, critic, log_std = S.policy(row.obs_dim, row.actor, row.act_dim, row.activation, seed=row.seed, normalize=S.row_normalize(index),
                                           critic_widths=row.critic, low=-R.ACTION_BOUND, high=R.ACTION_BOUND)
    return pol, actor


def _trainer(pol, **kw):
    from upkie_amd.distill import DistillTrainer

    return DistillTrainer(pol, **kw)


def _unchanged_words(pol, tr, packed0):
    """log_std, every critic word and the fixed words are the bits they were, and their moments exactly zero. The actor's
    words are found through the policy's own packing index (which source tensor every packed word is gathered from)."""
    sizes = [t.numel() for t in pol.sources()]
    owner = torch.full((sum(sizes) + 1,), -1, dtype=torch.long, device=DEV)  # (the last slot: padding)
    start = 0
    for k, n in enumerate(sizes):
        owner[start:start + n] = k
        start += n
    word_owner = owner[pol._index.long()]
    nf = pol.n_fixed
    first, last = nf + 1, nf + 2 * (int(pol.shape.actor_layers) + 1)  # (the actor's tensors in sources(): after log_std)
    actor = (word_owner >= first) & (word_owner <= last)
    at = torch.nonzero(actor).reshape(-1)
    outside = torch.ones_like(actor)
    outside[int(at.min()):int(at.max()) + 1] = False  # (the actor's span, its padding words included)
    for k in list(range(first)) + list(range(last + 1, len(sizes))):
        assert bool(outside[word_owner == k].all()), f"source {k} lies outside the actor's span"
    assert torch.equal(pol.packed[outside].view(torch.int32), packed0[outside].view(torch.int32)), "log_std, the critic, the fixed words: same bits"
    assert not bool(tr.m[outside].any()) and not bool(tr.v[outside].any()), "their moments are exactly zero"
    assert not bool(tr.m[~outside][word_owner[~outside] < 0].any()), "padding words inside the span have a zero gradient"


# ---------------------------------------------------------------- the gradient launch
@pytest.mark.parametrize("index,row", ROWS)
def test_gradient_against_the_fp64_twin(index, row):
    """One minibatch of all T N samples, no clipping (max_grad_norm 1e9): Adam's first moment is (1 - beta1) g."""
    N, D, A = row.N, row.obs_dim, row.act_dim
    total = T * N
    shape, sources, obs, labels = R.gradient_case(index, row)
    pol, actor = _student(index, row)
    for k, (a, b) in enumerate(zip(sources, S.sources_of(pol))):
        if k not in (2, 3, 4):  # (action bounds and log_std: float32 on the device)
            assert np.array_equal(np.asarray(a).reshape(-1), b.reshape(-1)), k
    src0 = S.sources_of(pol)
    d_obs, d_labels = torch.as_tensor(obs, device=DEV).reshape(T, N, D), torch.as_tensor(labels, device=DEV).reshape(T, N, A)
    assert np.median(np.abs(R.mean_of(shape, src0, obs) - labels)) >= 0.1, "the labels are far from the student's mean"
    # torch fp32 on the device, before the update writes the trained weights back into the modules: the row's own distance to the twin
    x = torch.as_tensor(R.normalized(shape, src0, obs), dtype=torch.float32, device=DEV)
    params = [p for m in actor if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]
    torch_grads = [np64(g) for g in torch.autograd.grad(nn.functional.mse_loss(actor(x), d_labels.reshape(total, A)), params)]
    tr = _trainer(pol, n_epochs=1, batch_size=total, max_grad_norm=1e9, seed=3)
    tr.prepare(d_obs, d_labels)
    packed0 = pol.packed.clone()
    state0 = [t.clone() for t in (pol.packed, tr.m, tr.v, tr.scalars)]
    stats = tr.update(d_obs, d_labels)
    torch.cuda.synchronize()
    idx = tr.perm[0].long().cpu().numpy()
    loss, grads, norm = R.minibatch(shape, src0, obs.astype(np.float64)[idx], labels.astype(np.float64)[idx])
    sl = R.actor_slice(shape)
    m = tr.state_dict()["m"]
    errors = [rel(np64(mm).reshape(g.shape) / float(BETA1_F32), g) for mm, g in zip(m[sl], grads[sl])]
    torch_errors = [rel(tg.reshape(g.shape), g) for tg, g in zip(torch_grads, grads[sl])]
    s = stats.double().cpu().numpy()[0, 0]
    plan = R.actor_plan(S.shape_of(row))  # (the launch's own geometry: the grid cap follows the actor's span)
    print(f"\ndistill gradient {S.row_id(row)} nw={plan['nw']} grad={max(errors):.3e} torch_grad={max(torch_errors):.3e} bound_grad={GRAD_BOUND:.0e} "
          f"loss_rel={abs(s[0] - loss) / loss:.3e} norm_rel={abs(s[1] - norm) / norm:.3e}")
    for k, e in enumerate(errors):
        assert e <= GRAD_BOUND, (k, e, torch_errors[k])
    np.testing.assert_allclose(s[:2], [loss, norm], rtol=1e-4, atol=1e-6)
    assert s[2] == 1.0, "nothing clipped"
    _unchanged_words(pol, tr, packed0)
    if plan["nw"] in (2, 3) or PR.chunks(plan, total) > plan["grid_cap"]:
        first = [t.clone() for t in (pol.packed, tr.m, tr.v, tr.scalars, stats)]
        for dst, src in zip((pol.packed, tr.m, tr.v, tr.scalars), state0):
            dst.copy_(src)
        again = tr.update(d_obs, d_labels, sync=False)
        torch.cuda.synchronize()
        for a, b in zip((pol.packed, tr.m, tr.v, tr.scalars, again), first):
            assert torch.equal(a, b), "two updates from the same state give the same bits"


# ---------------------------------------------------------------- one full update
def _case_row(case):
    N, D, widths, A, act = case
    return S.Row(N, D, list(widths), A, list(widths), act, "", 2 if N == 1 else 0)


def _check_full_update(pol, shape, src0, obs, labels):
    """One full update of 2 epochs x 3 minibatches (the last one short) at lr 1e-3 from a fresh optimiser, held to
    `distill_reference.update` on the trainer's own permutations: the statistics row of EVERY minibatch at the tolerance
    of tests/test_ppo_gpu.py's statistics (rtol 1e-4, atol 1e-6); the parameters under the bound of its
    test_one_full_update_against_the_fp64_twin (`distill_reference.step_bound`: what a gradient error of the gradient
    test's bound moves one Adam step by), word by word, summed over the six steps as the fit test below sums it; the
    moments; the words that get no gradient. Then a second update whose clip bites at every minibatch, the same checks,
    the bound summed on. Minibatches 2 and 3 of an epoch start past 0 and the third is shorter than the workspace's
    layout: a launch that lost `minibatch_start`, or took the layout's size for the minibatch's, fails the rows."""
    lr, total = 1e-3, len(obs)
    D, A = obs.shape[1], labels.shape[1]
    d_obs, d_labels = torch.as_tensor(obs, device=DEV).reshape(T, -1, D), torch.as_tensor(labels, device=DEV).reshape(T, -1, A)
    batch = (total + 2) // 3
    packed0 = pol.packed.clone()
    sl = R.actor_slice(shape)
    params_start = R.trainable(shape, src0)
    parted = [0 * p for p in params_start]
    src, worst = src0, 0.0
    for max_grad_norm, seed in ((1.0, 5), (1e-3, 6)):
        tr = _trainer(pol, lr=lr, n_epochs=2, batch_size=batch, max_grad_norm=max_grad_norm, seed=seed)
        stats = tr.train(d_obs, d_labels)
        torch.cuda.synchronize()
        perms = [tr.perm[e].long().cpu().numpy() for e in range(2)]
        trace = []
        src, (m, v, t), ref_stats, _ = R.update(shape, src, obs, labels, perms, batch, lr=lr, max_grad_norm=max_grad_norm, trace=trace)
        assert tr.n_minibatches == -(-total // batch) and ref_stats.shape == (2, tr.n_minibatches, 3)
        assert total < 3 or (tr.n_minibatches == 3 and total - 2 * batch <= batch)
        sd = tr.state_dict()
        assert sd["t"] == t == 2 * tr.n_minibatches and sd["lr"] == pytest.approx(lr)
        np.testing.assert_allclose(stats.double().cpu().numpy(), ref_stats, rtol=1e-4, atol=1e-6)
        assert max_grad_norm == 1.0 or np.all(ref_stats[:, :, 2] < 1.0), "the clip bites at every minibatch"
        for p0, grads, coef in trace:
            parted = [d + R.step_bound(p, g, coef, lr) for d, p, g in zip(parted, p0, grads)]
        got = [np64(p) for p in pol.sources()[pol.n_fixed:]]
        for k, (p1, pr, bound) in enumerate(zip(got, R.trainable(shape, src), parted)):
            err = np.abs(p1.reshape(pr.shape) - pr)
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (k, max_grad_norm, worst)
        for got_s, want in ((sd["m"], m), (sd["v"], v)):
            for a, b in zip(got_s[sl], want[sl]):
                assert rel(np64(a).reshape(b.shape), b) <= 1e-4
        _unchanged_words(pol, tr, packed0)
    assert any(np.any(a != b) for a, b in zip(R.trainable(shape, src)[sl], params_start[sl])), "the update moved the actor"
    return worst


@pytest.mark.parametrize("case", S.CASES, ids=S.IDS)
def test_one_full_update_against_the_fp64_twin(case):
    index = S.CASES.index(case)
    row = _case_row(case)
    shape, sources, obs, labels = R.gradient_case(index, row)
    pol, _ = _student(index, row)
    worst = _check_full_update(pol, shape, S.sources_of(pol), obs, labels)
    print(f"\ndistill update {S.row_id(row)} worst |step - twin| / bound = {worst:.3e}")


def test_one_full_update_of_an_asymmetric_student():
    """The critic reads rows of its own (12 words, the actor 5): the update needs none of them and moves no critic word."""
    index, row = 5, AS.ROWS[5]
    normalize = AS.row_normalize(index)
    pol, _, _, _ = AS.policy(row, normalize=normalize, low=-R.ACTION_BOUND, high=R.ACTION_BOUND)
    assert pol.asymmetric and int(pol.shape.critic_obs_dim) == 12
    src0 = S.sources_of(pol)
    obs = AS.row_observations(row, seed=7, steps=T)[0].numpy().reshape(T * row.N, row.obs_dim)
    teacher = AS.Row(*row[:-1], seed=row.seed + 100)
    labels = (R.mean_of(pol.shape, AS.row_sources(teacher, *AS.row_modules(teacher), normalize), obs)
              + np.random.default_rng(9).normal(0.0, R.LABEL_NOISE, size=(len(obs), row.act_dim))).astype(np.float32)
    assert np.median(np.abs(R.mean_of(pol.shape, src0, obs) - labels)) >= 0.1
    worst = _check_full_update(pol, pol.shape, src0, obs, labels)
    print(f"\ndistill update asymmetric {AS.row_id(row)} worst |step - twin| / bound = {worst:.3e}")


# ---------------------------------------------------------------- determinism, graph replay
@pytest.mark.parametrize("case", [S.CASES[0], S.CASES[2], S.CASES[4]], ids=[S.IDS[0], S.IDS[2], S.IDS[4]])
def test_deterministic_and_graph_replay_bit_identical(case):
    index, row = S.CASES.index(case), _case_row(case)
    _, _, obs, labels = R.gradient_case(index, row)
    pol, _ = _student(index, row)
    d_obs, d_labels = torch.as_tensor(obs, device=DEV), torch.as_tensor(labels, device=DEV)
    tr = _trainer(pol, n_epochs=2, batch_size=(len(obs) + 2) // 3, seed=1)
    tr.prepare(d_obs, d_labels)
    kept = (pol.packed, tr.m, tr.v, tr.scalars)
    s0 = [t.clone() for t in kept]

    def restore():
        for dst, src in zip(kept, s0):
            dst.copy_(src)

    runs = []
    for _ in range(2):
        restore()
        stats = tr.update(d_obs, d_labels, sync=False).clone()
        torch.cuda.synchronize()
        runs.append([t.clone() for t in kept] + [stats])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], s0[0]), "training moved the weights"
    restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr.update(d_obs, d_labels, sync=False)
    restore()  # (capture records, it does not run)
    tr.stats.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(list(kept) + [tr.stats], runs[0]):
        assert torch.equal(a, b)
    # no partial, loss sum, folded gradient or square sum is read before this update wrote it: behind the header (the fold's
    # counter, zeroed once) the workspace may hold anything, here NaN bits
    restore()
    tr.workspace[256:].fill_(255)
    assert bool(torch.isnan(tr.workspace[256:260].view(torch.float32)).all())
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(list(kept) + [tr.stats], runs[0]):
        assert torch.equal(a, b)
    # the learning-rate word is followed without a re-capture: a replay at lr 0 moves no weight but counts its steps
    t_before, packed = float(tr.scalars[1]), pol.packed.clone()
    tr.set_lr(0.0)
    graph.replay()
    torch.cuda.synchronize()
    assert float(tr.scalars[1]) == t_before + tr.n_epochs * tr.n_minibatches and torch.equal(pol.packed, packed)
    tr.set_lr(1e-4)
    graph.replay()
    torch.cuda.synchronize()
    assert float(tr.scalars[0]) == 1e-4 and not torch.equal(pol.packed, packed)


# ---------------------------------------------------------------- the mix
def _mix(num_envs, act_dim, offset, beta=0.0):
    """A simulation handle that is never stepped, and the mix on it."""
    from upkie_amd.distill import DaggerMix
    from upkie_amd.model.default_model import default_model
    from upkie_amd.sim import BatchedSim

    cfg = abi.default_sim_config(num_envs, seed=R.MIX_SEED)
    cfg.env_id_offset = offset
    sim = BatchedSim(cfg, default_model())
    low, high = R.mix_bounds(act_dim)
    return sim, DaggerMix(sim, act_dim, low, high, beta)


@pytest.mark.parametrize("num_envs,act_dim", R.mix_cases())
def test_the_mix_is_the_twin_after_every_call(num_envs, act_dim):
    sim, mix = _mix(num_envs, act_dim, R.MIX_OFFSET)
    low, high = R.mix_bounds(act_dim)
    for beta in R.MIX_BETAS:
        mix.reset()
        mix.set_beta(beta)
        twin = R.MixTwin(num_envs, low, high, seed=R.MIX_SEED, env_id_offset=R.MIX_OFFSET, beta=beta)
        teacher_rows = 0
        for c in range(R.MIX_CALLS):
            label, student = R.mix_inputs(num_envs, act_dim, c, R.MIX_OFFSET)
            applied = mix.step(torch.from_numpy(label).to(DEV), torch.from_numpy(student).to(DEV))
            want, drove = twin.step(label, student)
            torch.cuda.synchronize()
            assert np.array_equal(mix.drove.cpu().numpy(), drove), (beta, c)
            assert np.array_equal(bits(applied.cpu().numpy()), bits(want)), (beta, c)
            assert np.array_equal(mix.calls.cpu().numpy().view(np.uint32), twin.calls), (beta, c)
            teacher_rows += int(drove.sum())
        assert teacher_rows == {0.0: 0, 1.0: R.MIX_CALLS * num_envs}.get(beta, teacher_rows)
        assert beta != 0.5 or 0 < teacher_rows < R.MIX_CALLS * num_envs
    sim.close()


def test_two_shards_of_32_are_one_batch_of_64_and_a_captured_loop_follows_beta():
    A = 3
    whole_sim, whole = _mix(64, A, R.MIX_OFFSET, 0.5)
    shards = [_mix(32, A, R.MIX_OFFSET + k, 0.5) for k in (0, 32)]
    for c in range(R.MIX_CALLS):
        label, student = (torch.from_numpy(a).to(DEV) for a in R.mix_inputs(64, A, c, R.MIX_OFFSET))
        whole.step(label, student)
        for k, (_, shard) in enumerate(shards):
            shard.step(label[32 * k:32 * k + 32].contiguous(), student[32 * k:32 * k + 32].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(torch.cat([s.applied for _, s in shards]), whole.applied) and torch.equal(torch.cat([s.drove for _, s in shards]), whole.drove)
    # a captured loop of four calls: the beta word moves between replays, the counters inside them
    label, student = (torch.from_numpy(a).to(DEV) for a in R.mix_inputs(64, A, 0, R.MIX_OFFSET))
    drove = torch.zeros(4, 64, dtype=torch.uint8, device=DEV)
    whole.reset()
    whole.step(label, student, drove[0])  # (warm-up off the capture)
    torch.cuda.synchronize()
    whole.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(4):
            whole.step(label, student, drove[k])
        with pytest.raises(Exception, match="outside a graph capture"):
            whole.set_beta(1.0)
    low, high = R.mix_bounds(A)
    twin = R.MixTwin(64, low, high, seed=R.MIX_SEED, env_id_offset=R.MIX_OFFSET)
    for beta in (0.5, 1.0, 0.0, 0.25):
        whole.set_beta(beta)
        twin.threshold = R.threshold(beta)
        graph.replay()
        torch.cuda.synchronize()
        want = np.stack([twin.step(*R.mix_inputs(64, A, 0, R.MIX_OFFSET))[1] for _ in range(4)])
        assert np.array_equal(drove.cpu().numpy(), want), beta
    for sim, _ in shards + [(whole_sim, None)]:
        sim.close()


# ---------------------------------------------------------------- the driver
B, STEPS, SEED = 64, 8, 5
STORED = ("observations", "labels", "drove")  # (what a rollout stores: part of every snapshot)


def _actor_critic(d_in, seed, dev, low=-1.0, high=1.0, **kw):
    from upkie_amd.policies import MlpActorCritic

    torch.manual_seed(seed)
    return MlpActorCritic.from_modules(tower(d_in, 1, 32).to(dev), tower(d_in, 1, 32).to(dev), nn.Parameter(torch.zeros(1, device=dev)),
                                       action_low=[low], action_high=[high], seed=seed, **kw)


def _make(staged=False, teacher_kind="mlp", **kw):
    """(env, student, teacher, model): the pendulum env, a teacher on the raw observation with frozen statistics of its
    own, and (``staged``) a student behind a pipeline with targets and events."""
    from upkie_amd.distill import Distillation

    env = pendulum(B, 6, seed=0)
    dev = env.device
    args = dict(n_steps=STEPS, n_epochs=2, batch_size=B * STEPS // 2, seed=SEED, beta=0.5)
    raw = 4
    if staged:
        from upkie_amd.events import EpisodeEvents
        from upkie_amd.pipeline import AgentPipeline
        from upkie_amd.targets import TaskTargets

        targets = TaskTargets(env, names=("ground_velocity",), ranges=[(-0.5, 0.5)], resample_steps=(2, 4))
        raw = targets.dim
        pipeline = AgentPipeline(B, raw, [-1.0], [1.0], dt=1.0 / 200.0, stack=2, observation_noise=[0.01] * raw, action_lag=0.05, seed=5, device=dev)
        args.update(targets=targets, pipeline=pipeline, events=EpisodeEvents(env, push_prob=0.5, push_norm=(5.0, 20.0), push_steps=(1, 3)))
        student = _actor_critic(pipeline.stacked_dim, 1, dev)
    else:
        student = _actor_critic(4, 1, dev)
    if teacher_kind == "linear":  # (the README gains' form: `Distillation` wraps it in a `LinearTeacher`)
        from upkie_amd.policies import LinearPolicy

        teacher = LinearPolicy(torch.linspace(0.5, 2.0, raw).reshape(raw, 1), clip=1.0, device=dev)
    elif teacher_kind == "privileged":  # (the teacher reads a row of its own: observation, command, the push that acts)
        from upkie_amd.privileged import PrivilegedObservation

        rows = PrivilegedObservation(env, events=args["events"], pipeline=args["pipeline"], include=("observation", "command", "push_force"))
        args["teacher_observation"] = rows
        teacher = _actor_critic(rows.dim, 2, dev)
    else:
        teacher = _actor_critic(raw, 2, dev, obs_mean=torch.linspace(-0.1, 0.1, raw), obs_var=torch.linspace(0.5, 1.5, raw), clip_obs=5.0)
    args.update(kw)
    return env, student, teacher, Distillation(env, student, teacher, **args)


ITERATIONS = 3
RECORD_KEYS = ("distill/loss", "distill/grad_norm", "distill/beta", "distill/teacher_drove_frac", "rollout/ep_rew_mean", "rollout/ep_len_mean",
               "time/total_timesteps", "time/iterations")


@pytest.mark.parametrize("staged", (False, True), ids=("plain", "pipeline-targets-events"))
def test_graphed_equals_eager_bit_for_bit(staged):
    schedule = dict(beta=lambda p: 0.25 + 0.5 * p, learning_rate=lambda p: 1e-3 * (0.5 + p))
    env, student, teacher, model = _make(staged, graph=True, **schedule)
    with env:
        model.learn(ITERATIONS * B * STEPS)
        graphed = snapshot(model, STORED)
    env, student, teacher, model = _make(staged, graph=False, **schedule)
    with env:
        warm_up_as_the_capture_does(model)
        model.learn(ITERATIONS * B * STEPS)
        eager = snapshot(model, STORED)
    assert all(k in graphed[0] for k in ("packed", "m", "v", "scalars", "mix.calls", "mix.threshold", "calls"))
    for k in graphed[0]:
        assert same(graphed[0][k], eager[0][k]), k
    assert same(graphed[1], eager[1]) and len(graphed[1]) == ITERATIONS
    for i, record in enumerate(graphed[1]):
        assert all(k in record for k in RECORD_KEYS), sorted(record)
        assert 0.0 < record["distill/teacher_drove_frac"] < 1.0 and record["distill/loss"] > 0.0
    # the schedules moved both device words between the replays, with no re-capture
    progress = [1.0] + [1.0 - float(k * B * STEPS) / float(ITERATIONS * B * STEPS) for k in (1, 2)]  # (what each rollout ran under)
    assert [r["distill/beta"] for r in graphed[1]] == [schedule["beta"](p) for p in progress]
    assert graphed[1][0]["distill/learning_rate"] > graphed[1][-1]["distill/learning_rate"]
    assert int(graphed[0]["mix.calls"][0]) == ITERATIONS * STEPS + 1, "the warm-up step, then STEPS per iteration"


@pytest.mark.parametrize("teacher_kind,staged", (("linear", False), ("privileged", True)))
def test_a_linear_and_a_privileged_teacher_survive_capture(teacher_kind, staged):
    """The `LinearTeacher` adapter and ``teacher_observation=PrivilegedObservation`` inside the captured rollout: graphed
    equals eager bit for bit, the labels are the teacher's on the rows it was given."""
    results = []
    for graph in (True, False):
        env, student, teacher, model = _make(staged, teacher_kind, graph=graph)
        with env:
            if not graph:
                warm_up_as_the_capture_does(model)
            model.learn(2 * B * STEPS)
            results.append(snapshot(model, STORED))
            torch.cuda.synchronize()
            if teacher_kind == "linear":
                assert type(model.teacher).__name__ == "LinearTeacher" and model.teacher_observation is None
                raw = model._agent.raw_observation  # (after the last step; the last label row was made one step before)
                assert raw.shape == (B, 4) and float(model.labels.abs().max()) <= 1.0 and float(model.labels.abs().sum()) > 0.0
            else:
                rows = model.teacher_observation
                assert rows.dim == 4 + 1 + 1 + 3 and int(teacher.shape.obs_dim) == rows.dim
                want = torch.empty(B, 1, device=DEV)
                teacher.mean(rows.observation, want)  # (the row after the last step: the label the next step would store)
                assert want.shape == model.labels[0].shape and float(model.labels.abs().sum()) > 0.0
                assert "teacher_observation.observation" in results[-1][0]
    for k in results[0][0]:
        assert same(results[0][0][k], results[1][0][k]), k
    assert same(results[0][1], results[1][1]) and len(results[0][1]) == 2


def test_a_run_saved_after_two_iterations_resumes_bit_for_bit(tmp_path):
    from upkie_amd.distill import Distillation

    path = str(tmp_path / "distill.pt")
    env, student, teacher, model = _make(True, graph=True)
    with env:
        model.learn(ITERATIONS * B * STEPS)
        whole = snapshot(model, STORED)
    env, student, teacher, model = _make(True, graph=True)
    with env:
        model.learn(ITERATIONS * B * STEPS, callback=lambda m, rec: m.iterations < 2)
        assert model.iterations == 2
        model.save(path)
    env, student, teacher, fresh = _make(True, graph=True)
    with env:
        resumed = Distillation.load(path, env, student, teacher, n_steps=STEPS, n_epochs=2, batch_size=B * STEPS // 2, seed=SEED, beta=0.5,
                                    targets=fresh.targets, pipeline=fresh.pipeline, events=fresh.events)
        resumed.learn(B * STEPS, reset_num_timesteps=False)
        end = snapshot(resumed, STORED)
    for k in whole[0]:
        assert same(whole[0][k], end[0][k]), k
    assert same(whole[1][2:], end[1])


@pytest.mark.parametrize("staged", (False, True), ids=("plain", "pipeline-targets-events"))
def test_the_buffer_holds_what_the_twins_give_on_the_recorded_observations(staged):
    """observations[t]: the student's row at step t (its pipeline's stack when staged), bit for bit; labels[t]: the
    teacher's fp64 mean twin on the raw row recorded at the same instant, within the mean's bound; drove[t]: the mix twin
    under the env's seed, bit for bit; the applied action: the clamp of the driver's row."""
    env, student, teacher, model = _make(staged, graph=False, normalize=False)
    with env:
        model._setup()
        agent, rows = model._agent, []
        step = model.mix.step

        def recording(label, student_action, drove):
            applied = step(label, student_action, drove)
            rows.append({"raw": agent.raw_observation.clone(), "seen": agent.observation.clone(), "action": student_action.clone(),
                         "applied": applied.clone()})
            return applied

        model.mix.step = recording
        model.collect_rollouts()
        torch.cuda.synchronize()
        src = S.sources_of(teacher)
        twin = R.MixTwin(B, [-1.0], [1.0], seed=SEED, beta=0.5)
        for t in range(STEPS):
            row = rows[t]
            assert torch.equal(model.observations[t], row["seen"]), t
            assert row["raw"].shape[1] == (5 if staged else 4) and row["seen"].shape[1] == (12 if staged else 4)
            want = R.mean_of(teacher.shape, src, np64(row["raw"]))
            assert np.abs(np64(model.labels[t]) - want).max() <= S.DEFAULT_BOUNDS["mean"], t
            applied, drove = twin.step(model.labels[t].cpu().numpy(), row["action"].cpu().numpy())
            assert np.array_equal(model.drove[t].cpu().numpy(), drove), t
            assert np.array_equal(bits(row["applied"].cpu().numpy()), bits(applied)), t
        assert 0 < int(model.drove.sum()) < B * STEPS


def test_ppo_takes_a_distilled_student_over_with_its_normaliser():
    from upkie_amd.ppo import Ppo

    env, student, teacher, model = _make(False, graph=True)
    with env, pendulum(32, 6, seed=0) as smaller:
        model.learn(2 * B * STEPS)
        statistics = model.normalizer.obs_mean.clone()
        with pytest.raises(ValueError, match=f"the policy's normaliser serves {B} envs at gamma 0.99, this run has 32 at 0.99"):
            Ppo(smaller, student, n_steps=STEPS, batch_size=32 * STEPS // 2)._setup()
        with pytest.raises(ValueError, match=f"this run has {B} at 0.9:"):
            Ppo(env, student, n_steps=STEPS, gamma=0.9, batch_size=B * STEPS // 2)._setup()
        packed = student.packed.clone()
        tuned = Ppo(env, student, n_steps=STEPS, n_epochs=2, batch_size=B * STEPS // 2, seed=SEED)
        tuned.learn(2 * B * STEPS)
        torch.cuda.synchronize()
        assert tuned.normalizer is model.normalizer and student._normalizer is model.normalizer
        assert not torch.equal(model.normalizer.obs_mean, statistics), "the statistics went on moving"
        assert not torch.equal(student.packed, packed) and bool(torch.isfinite(student.packed).all())
        assert len(tuned.records) == 2 and all(r["train/loss"] == r["train/loss"] for r in tuned.records)


def test_an_eval_callback_leaves_the_run_alone():
    from upkie_amd.evaluation import EvalCallback

    def learn(with_callback):
        env, student, teacher, model = _make(False, graph=True)
        with env, pendulum(32, 6, seed=9) as eval_env:
            callback = EvalCallback(eval_env, n_eval_episodes=48, eval_freq=STEPS, seed=9, chunk=4) if with_callback else None
            model.learn(2 * B * STEPS, callback=callback)
            if with_callback:
                assert len(callback.evaluations["timesteps"]) == 2 and all("eval/mean_reward" in r for r in model.records)
            return snapshot(model, STORED)

    plain, evald = learn(False), learn(True)
    for k in plain[0]:
        assert same(plain[0][k], evald[0][k]), k
    strip = lambda records: [{k: v for k, v in r.items() if not k.startswith("eval/")} for r in records]  # noqa: E731
    assert same(strip(plain[1]), strip(evald[1]))


@pytest.mark.parametrize("beta", (0.0, 1.0))
def test_at_the_ends_of_beta_one_driver_has_every_env(beta):
    env, student, teacher, model = _make(False, graph=False, beta=beta, normalize=False)
    with env:
        model._setup()
        applied, step = [], model.mix.step

        def recording(label, student_action, drove):
            out = step(label, student_action, drove)
            applied.append((out.clone(), label.clone(), student_action.clone()))
            return out

        model.mix.step = recording
        model.collect_rollouts()
        torch.cuda.synchronize()
        assert bool((model.drove == int(beta)).all())
        differ = 0
        for out, label, action in applied:
            assert torch.equal(out, (label if beta == 1.0 else action).clamp(-1.0, 1.0))
            differ += int((label.clamp(-1.0, 1.0) != action.clamp(-1.0, 1.0)).sum())
        assert differ > B, "the two drivers' rows differ, so the check tells them apart"


def test_fifty_full_batch_updates_follow_the_twins_loss_curve():
    """A fixed dataset labelled by a teacher; a student of the teacher's architecture from another seed; 50 updates of one
    full batch each. The device's loss at update k is held to the twin's within the loss statistic's tolerance (rtol 1e-4,
    atol 1e-6) plus what the parameters may have parted by: the one-step bound of the full-update test, word by word,
    summed over the updates before k and carried to the loss through |d loss / d word| (first order; the twin's gradient).
    Whether the fit works is the twin's to say, on the CPU: its last loss is below its first."""
    row = S.Row(256, 5, [40, 24], 3, [40, 24], "tanh", "", 0)
    normalize, updates, lr = False, 50, 1e-3
    shape = S.shape_of(row)
    pol, _, _, _ = S.policy(row.obs_dim, row.actor, row.act_dim, row.activation, seed=row.seed, critic_widths=row.critic)
    src = S.sources_of(pol)
    obs = S.row_observations(row, seed=11).numpy()
    labels = R.mean_of(shape, R.teacher_sources(row, normalize), obs).astype(np.float32)
    d_obs, d_labels = torch.as_tensor(obs, device=DEV), torch.as_tensor(labels, device=DEV)
    tr = _trainer(pol, lr=lr, n_epochs=1, batch_size=row.N, max_grad_norm=1.0, seed=0)
    device_loss = []
    for _ in range(updates):
        device_loss.append(tr.train(d_obs, d_labels, sync=False)[0, 0].clone())
    torch.cuda.synchronize()
    device_loss = torch.stack(device_loss).double().cpu().numpy()[:, 0]
    state, identity = None, [np.arange(row.N)]  # (one full batch: its order does not matter to the twin)
    parted = [0 * p for p in R.trainable(shape, src)]
    worst = 0.0
    twin_loss = []
    for k in range(updates):
        params0 = R.trainable(shape, src)
        src, state, stats, grads = R.update(shape, src, obs, labels, identity, row.N, lr=lr, max_grad_norm=1.0, state=state)
        loss, coef = stats[0, 0, 0], stats[0, 0, 2]
        twin_loss.append(loss)
        bound = 1e-4 * abs(loss) + 1e-6 + sum(float(np.sum(np.abs(g) * d)) for g, d in zip(grads, parted))
        worst = max(worst, abs(device_loss[k] - loss) / bound)
        assert abs(device_loss[k] - loss) <= bound, (k, device_loss[k], loss, bound)
        parted = [d + R.step_bound(p0, g, coef, lr) for d, p0, g in zip(parted, params0, grads)]
    print(f"\ndistill fit loss {twin_loss[0]:.4e} -> {twin_loss[-1]:.4e} (twin), device last {device_loss[-1]:.4e}, worst |device - twin| / bound = {worst:.3e}")
    assert twin_loss[-1] < twin_loss[0], "the twin's fit works"
    assert int(tr.state_dict()["t"]) == updates


def test_the_example_runs():
    env = dict(os.environ, EXAMPLE_ENVS="64", EXAMPLE_STEPS="8", EXAMPLE_ITERATIONS="2")
    result = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "distill_student.py")], capture_output=True, text=True, timeout=300, env=env,
                            cwd=os.path.join(ROOT, "examples"))
    assert result.returncode == 0, result.stderr[-3000:]
    out = result.stdout
    assert "teacher" in out and "distill/loss" in out and "fine-tune" in out and "nan" not in out.lower(), out
