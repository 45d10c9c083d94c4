"""The asymmetric actor-critic on the MI355X: the policy launch, the time-limit bootstrap and the PPO gradient launch with
a critic observation of its own against the composed fp64 twins (tests/asymmetric_reference.py) on every row of
tests/asymmetric_shapes.py; the degenerate case (Dc = D, the same rows and statistics) bit for bit against the symmetric
policy, a full update included; the privileged stage against its twin call by call, eager and replayed from a graph,
at the default layout and at every other layout of the table (orders, subsets, 256-word rows, 27 staged columns, masked
resets, steps without final_obs or end flags);
and `Ppo(critic_observation=...)` graphed against eager, saved and resumed, with the buffer's rows against the twin.
tests/test_asymmetric_critic.py shows on the host that these inputs tell the feature from its likely bugs.

Each twin test prints `asymmetric <family> <id> <figure>=<value> ...` before it asserts."""

import copy
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import asymmetric_reference as AR
from tests import asymmetric_shapes as AS
from tests import mlp_shapes as S
from tests import ppo_reference as PR
from tests.training_rig import np64, pendulum, pitch_reward, rel, same, snapshot, tower
from upkie_amd.ppo import PpoTrainer, trainable_offset
from upkie_amd.rollout import RolloutBuffer

pytestmark = pytest.mark.gpu
DEV = AS.DEV
T = AS.T
BETA1_F32 = np.float32(1.0) - np.float32(0.9)
ROWS = [pytest.param(i, r, id=AS.row_id(r)) for i, r in enumerate(AS.ROWS)]
BOUND = AS.BOUNDS


def _report(family, row, **figures):
    print(f"\nasymmetric {family} {AS.row_id(row)} " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------- 1. policy launch
@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("index,row", ROWS)
def test_policy_against_the_twin(index, row, normalize):
    N, D, A, Dc = row.N, row.obs_dim, row.act_dim, row.critic_obs_dim
    log_std = torch.linspace(-1.0, 0.5, A, device=DEV)
    pol, _, _, _ = AS.policy(row, normalize, log_std=log_std, low=-0.7, high=0.4)
    assert pol.asymmetric and pol.critic_obs_dim == Dc and int(pol.shape.normalize) == int(normalize)
    host = AS.row_sources(row, *AS.row_modules(row), normalize)
    for k, (a, b) in enumerate(zip(host, S.sources_of(pol))):
        if k not in (2, 3, 6):  # (action bounds and log_std are the test's own)
            assert np.array_equal(np.asarray(a).reshape(-1), b.reshape(-1)), k
    obs, cobs = (t.to(DEV) for t in AS.row_observations(row, scale=2.0 if normalize else 1.0))
    mean, norm, cnorm = torch.empty(N, A, device=DEV), torch.empty(N, D, device=DEV), torch.empty(N, Dc, device=DEV)
    env_action, action, value, log_prob = pol.act(obs, deterministic=True, out={"mean": mean, "norm_obs": norm, "norm_critic_obs": cnorm},
                                                  critic_obs=cobs)
    torch.cuda.synchronize()
    x64, m64, xc64, v64 = AR.forward(pol.shape, S.sources_of(pol), np64(obs), np64(cobs))
    err = {"mean": np.abs(np64(mean) - m64).max(), "value": np.abs(np64(value) - v64).max(), "norm_obs": np.abs(np64(norm) - x64).max(),
           "norm_critic_obs": np.abs(np64(cnorm) - xc64).max()}
    from tests import mlp_reference as R

    err["log_prob"] = np.abs(np64(log_prob) - R.log_prob(m64, m64, np64(log_std))).max()
    _report("policy", row, normalize=normalize, **{k: float(v) for k, v in err.items()})
    assert err["norm_obs"] <= BOUND["norm_obs"] and err["norm_critic_obs"] <= BOUND["norm_obs"]
    assert err["mean"] <= BOUND["mean"]
    assert err["value"] <= BOUND["value"]
    assert err["log_prob"] <= BOUND["log_prob"]
    assert torch.equal(action, mean) and torch.equal(env_action, mean.clamp(-0.7, 0.4))
    # the actor's outputs are the bits of a second launch that does not run the critic (value = NULL)
    again = {name: torch.full_like(t, float("nan")) for name, t in (("mean", mean), ("norm_obs", norm), ("action", action),
                                                                       ("env_action", env_action), ("log_prob", log_prob))}
    pol._launch(obs, True, again, critic_obs=cobs)
    fused = value.clone()
    v_only = pol.value(cobs, out=torch.full((N,), float("nan"), device=DEV))
    torch.cuda.synchronize()
    for name, t in (("mean", mean), ("norm_obs", norm), ("action", action), ("env_action", env_action), ("log_prob", log_prob)):
        assert torch.equal(_bits(again[name]), _bits(t)), name
    assert torch.equal(_bits(v_only), _bits(fused)), "the value-only launch gives the fused launch's bits"
    out = torch.full((N, A), float("nan"), device=DEV)
    assert torch.equal(_bits(pol.mean_action(obs, out)), _bits(env_action)), "mean_action needs no critic rows"
    with pytest.raises(ValueError, match=f"{Dc} words.*{D}"):
        pol.act(obs)
    if Dc != D:
        with pytest.raises(ValueError, match=f"{Dc} words per env"):
            pol.value(obs)


# ---------------------------------------------------------------- 2. the degenerate case, bit for bit
def _twins_of_one_network(row):
    """(symmetric policy, asymmetric policy with Dc = D): the same modules, the same statistics in both blocks."""
    from upkie_amd.policies import MlpActorCritic

    D, A = row.obs_dim, row.act_dim
    torch.manual_seed(row.seed)
    actor, critic = S.tower(D, row.actor, A, row.activation).to(DEV), S.tower(D, row.critic, 1, row.activation).to(DEV)
    mean, var = S.normalizer_stats(D, row.seed)
    out = []
    for asym in (False, True):
        a, c = copy.deepcopy(actor), copy.deepcopy(critic)
        kw = dict(critic_obs_mean=mean, critic_obs_var=var, asymmetric=True) if asym else {}
        log_std = nn.Parameter(torch.full((A,), -0.5, device=DEV))
        out.append(MlpActorCritic.from_modules(a, c, log_std, torch.full((A,), -1.0), torch.full((A,), 1.0), obs_mean=mean, obs_var=var,
                                               clip_obs=3.0, seed=7, **kw))
    return out


@pytest.mark.parametrize("index", AS.DEGENERATE, ids=[AS.row_id(AS.ROWS[i]) for i in AS.DEGENERATE])
def test_the_degenerate_case_is_the_symmetric_policy_bit_for_bit(index):
    row = AS.ROWS[index]
    N, D, A = row.N, row.obs_dim, row.act_dim
    sym, asym = _twins_of_one_network(row)
    assert not sym.asymmetric and asym.asymmetric and asym.critic_obs_dim == D
    off_s, off_a = trainable_offset(sym.shape), trainable_offset(asym.shape)
    assert off_a == off_s + 2 * ((D + 3) // 4 * 4) and torch.equal(sym.packed[off_s:], asym.packed[off_a:])
    obs = AS.row_observations(row, scale=2.0)[0].to(DEV)
    outs = []
    for pol in (sym, asym):
        extra = {"mean": torch.empty(N, A, device=DEV), "norm_obs": torch.empty(N, D, device=DEV)}
        kw = dict(critic_obs=obs) if pol.asymmetric else {}
        got = [t.clone() for t in pol.act(obs, out=extra, **kw)] + [extra["mean"], extra["norm_obs"]]
        reward = torch.linspace(-1.0, 1.0, N, device=DEV)
        truncated = (torch.arange(N, device=DEV) % 3 == 0).to(torch.uint8)
        terminated = (torch.arange(N, device=DEV) % 6 == 0).to(torch.uint8)
        got.append(pol.bootstrap_time_limits(obs, terminated, truncated, reward, 0.97).clone())
        outs.append(got)
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(_bits(a), _bits(b)), k

    # one full update: 2 epochs x 2 minibatches, the last one short
    data = S.row_rollout(S.Row(N, D, row.actor, A, row.critic, row.activation, "", row.seed), sym.shape, S.sources_of(sym))
    total = T * N
    results = []
    for pol in (sym, asym):
        buf = RolloutBuffer(T, N, obs_shape=(D,), action_shape=(A,), device=DEV, critic_obs_shape=(D,) if pol.asymmetric else None)
        for name in ("observations", "actions", "values", "log_probs"):
            getattr(buf, name).copy_(torch.as_tensor(data[name], device=DEV).reshape(getattr(buf, name).shape))
        if pol.asymmetric:
            buf.critic_observations.copy_(buf.observations)
        buf.advantages, buf.returns = torch.as_tensor(data["advantages"], device=DEV), torch.as_tensor(data["returns"], device=DEV)
        buf.pos, buf.full = T, True
        tr = PpoTrainer(pol, n_epochs=2, batch_size=N + 7, ent_coef=0.01, clip_range_vf=0.2, seed=3)
        stats = tr.train(buf)
        torch.cuda.synchronize()
        assert tr.n_minibatches == 2 and total - (N + 7) < N + 7
        off = trainable_offset(pol.shape)
        results.append((pol.packed[off:].clone(), tr.m[off:].clone(), tr.v[off:].clone(), stats.clone(), tr.scalars.clone(),
                        torch.tensor(tr.workspace.numel()), [p.detach().clone() for p in pol._params]))
    for k, (a, b) in enumerate(zip(*results)):
        if isinstance(a, list):
            assert all(torch.equal(x, y) for x, y in zip(a, b)), "the modules' parameters after the write-back"
        else:
            assert torch.equal(a, b), ("packed", "m", "v", "stats", "scalars", "workspace bytes")[k]
    assert float(results[0][4][1]) == 4.0 and float(results[0][1].abs().sum()) > 0.0, "four optimiser steps were taken"


# ---------------------------------------------------------------- 3. time-limit bootstrap
@pytest.mark.parametrize("index,row", ROWS)
def test_bootstrap_is_the_value_of_the_final_critic_row(index, row):
    N = row.N
    pol, _, _, _ = AS.policy(row, AS.row_normalize(index))
    _, final = (t.to(DEV) for t in AS.row_observations(row, seed=11, scale=1.5))
    g = torch.Generator().manual_seed(index)
    truncated = (torch.rand(N, generator=g) < 0.4).to(torch.uint8).to(DEV)
    terminated = (torch.rand(N, generator=g) < 0.3).to(torch.uint8).to(DEV)
    truncated[0] = 1
    terminated[0] = 0
    reward0 = torch.randn(N, generator=g).to(DEV)
    value = pol.value(final, out=torch.empty(N, device=DEV)).clone()
    reward = pol.bootstrap_time_limits(final, terminated, truncated, reward0.clone(), 0.97)
    torch.cuda.synchronize()
    boot = (truncated != 0) & (terminated == 0)
    want = torch.where(boot, reward0 + torch.tensor(0.97, dtype=torch.float32, device=DEV) * value, reward0)
    assert torch.equal(_bits(reward), _bits(want)), "reward + fl(gamma * value(final critic row)) where truncated, untouched elsewhere"
    assert int(boot.sum()) >= 1 and (int((~boot).sum()) >= 1 or N == 1)
    _, _, _, v64 = AR.forward(pol.shape, S.sources_of(pol), np.zeros((N, row.obs_dim)), np64(final))
    assert np.abs(np64(value) - v64).max() <= BOUND["value"]


# ---------------------------------------------------------------- 4. PPO gradient launch
def _buffer(row, data):
    buf = RolloutBuffer(T, row.N, obs_shape=(row.obs_dim,), action_shape=(row.act_dim,), device=DEV, critic_obs_shape=(row.critic_obs_dim,))
    for name in ("observations", "critic_observations", "actions", "values", "log_probs"):
        getattr(buf, name).copy_(torch.as_tensor(data[name], device=DEV).reshape(getattr(buf, name).shape))
    buf.advantages, buf.returns = torch.as_tensor(data["advantages"], device=DEV), torch.as_tensor(data["returns"], device=DEV)
    buf.pos, buf.full = T, True
    return buf


def _first_minibatch(tr, buf, size):
    """Epoch 0's advantage statistics and its first minibatch alone (gradient, fold, Adam): what `PpoTrainer.update` issues
    first. Returns that minibatch's stats row."""
    total = T * buf.n_envs
    head = (C.byref(tr.policy.shape), C.byref(tr.config))
    from upkie_amd.launch import ptr

    data = tuple(ptr(t) for t in (buf.observations, buf.critic_observations, buf.actions, buf.values, buf.log_probs, tr.advantages, tr.returns))
    with torch.cuda.device(tr.device):
        tr._advantage_stats(0, total, ptr(tr.perm[0]), data[-2])
        tr._minibatch(0, 0, head, total, 0, size, ptr(tr.perm[0]), data)
    torch.cuda.synchronize()
    return tr.stats[0, 0]


@pytest.mark.parametrize("short,obs_normalized", [(False, False), (True, True)], ids=["TN-raw", "TN-7-normalized"])
@pytest.mark.parametrize("index,row", ROWS)
def test_gradient_against_the_twin(index, row, short, obs_normalized):
    """One minibatch of T N (or T N - 7) samples of a normalising policy, no gradient clipping: every gradient tensor against
    the composed fp64 twin (read from Adam's m after one step), the statistics row, and the same bits from the same state."""
    N, D, A, Dc = row.N, row.obs_dim, row.act_dim, row.critic_obs_dim
    total = T * N
    size = total - min(7, total - 1) if short else total  # (the N = 1 row has two samples: its short minibatch is one of them)
    log_std = nn.Parameter(torch.full((A,), -0.5, device=DEV))
    pol, _, _, _ = AS.policy(row, normalize=True, log_std=log_std)
    src0 = S.sources_of(pol)
    data = AS.row_rollout(row, pol.shape, src0, obs_normalized=obs_normalized)
    buf = _buffer(row, data)
    tr = PpoTrainer(pol, n_epochs=1, batch_size=size, max_grad_norm=1e9, ent_coef=0.01, clip_range_vf=0.2, seed=3, obs_normalized=obs_normalized)
    tr.prepare(buf)
    state0 = [t.clone() for t in (pol.packed, tr.m, tr.v, tr.control)]
    stats = _first_minibatch(tr, buf, size).clone()
    idx = tr.perm[0].long().cpu().numpy()[:size]
    flat = lambda k, *tail: data[k].astype(np.float64).reshape(total, *tail)[idx]  # noqa: E731
    ref_stats, ref_grads, ratio = AR.minibatch(pol.shape, src0, flat("observations", D), flat("critic_observations", Dc), flat("actions", A),
                                               flat("values"), flat("log_probs"), flat("advantages"), flat("returns"),
                                               obs_normalized=obs_normalized, ent_coef=0.01, clip_range_vf=0.2, max_grad_norm=1e9)
    for edge in (0.8, 1.2):
        assert not (np.abs(ratio - edge) < 1e-4).any(), "no sample's ratio within 1e-4 of a clip bound"
    m = tr.state_dict()["m"]
    assert len(m) == len(ref_grads)
    errors = [rel(np64(mm).reshape(g.shape) / float(BETA1_F32), g) for mm, g in zip(m, ref_grads)]
    worst = int(np.argmax(errors))
    plan = AR.plan(pol.shape)
    _report("gradient", row, size=size, obs_normalized=obs_normalized, W=AR.layout(pol.shape)["W"], nw=plan["nw"], chunks=PR.chunks(plan, size),
            grid_cap=plan["grid_cap"], worst_tensor=worst, grad=float(errors[worst]), critic_first_layer=float(errors[1 + 2 * (len(row.actor) + 1)]), bound_grad=BOUND["grad"])
    for k, e in enumerate(errors):
        assert e <= BOUND["grad"], (k, e)
    s = stats.double().cpu().numpy()
    np.testing.assert_allclose(s[[0, 1, 2, 3, 6]], ref_stats[[0, 1, 2, 3, 6]], rtol=1e-4, atol=1e-6)
    assert abs(s[4] - ref_stats[4]) <= 1e-5 and abs(s[5] - ref_stats[5]) <= 1.0 / size

    first = [t.clone() for t in (pol.packed, tr.m, tr.v, tr.control)]
    for dst, src in zip((pol.packed, tr.m, tr.v, tr.control), state0):
        dst.copy_(src)
    again = _first_minibatch(tr, buf, size)
    for a, b in zip((pol.packed, tr.m, tr.v, tr.control, again), first + [stats]):
        assert torch.equal(a, b), "two runs from the same state give the same bits"
    assert not torch.equal(pol.packed, state0[0]), "the update moved the weights"


def test_the_trainer_names_both_sizes_on_every_mismatch():
    row = AS.ROWS[0]
    pol, _, _, _ = AS.policy(row)
    sym, _, _, _ = S.policy(row.obs_dim, row.actor, row.act_dim, row.activation)
    mk = lambda shape: RolloutBuffer(T, row.N, obs_shape=(row.obs_dim,), action_shape=(row.act_dim,), device=DEV, critic_obs_shape=shape)  # noqa: E731
    for policy, shape, pattern in ((pol, None, "asymmetric.*5 words.*actor 3.*critic_obs_shape"), (sym, (5,), "5 words.*symmetric.*3-word"),
                                   (pol, (4,), "4 critic observation words.*takes 5")):
        buf = mk(shape)
        buf.advantages = buf.returns = torch.zeros(T, row.N, device=DEV)
        with pytest.raises(ValueError, match=pattern):
            PpoTrainer(policy).prepare(buf)
    from upkie_amd.normalize import RunningNormalizer

    with pytest.raises(ValueError, match="critic takes 5 observation words, the normalizer 3"):
        RunningNormalizer(row.N, 3, device=DEV).attach(pol, tower="critic")
    with pytest.raises(ValueError, match="needs an asymmetric policy.*3-word.*5 columns"):
        RunningNormalizer(row.N, 5, device=DEV).attach(sym, tower="critic")
    norm = RunningNormalizer(row.N, 5, norm_reward=False, clip_obs=3.0, device=DEV)
    norm.attach(pol, tower="critic")
    rows = AS.row_observations(row)[1].to(DEV)
    norm.reset(rows)
    torch.cuda.synchronize()
    at = pol.critic_stats_offset()
    assert torch.equal(pol.packed[at:at + 5], norm.obs_mean_f32) and torch.equal(pol.packed[at + 8:at + 13], norm.obs_std_f32)
    assert torch.equal(pol.sources()[4], norm.obs_mean_f32) and float(norm.obs_mean_f32.abs().sum()) > 0.0
    assert torch.equal(pol.packed[:3], torch.zeros(3, device=DEV)), "the actor's statistics are not the critic normaliser's to write"


# ---------------------------------------------------------------- 5. the privileged stage
def _stage(num_envs, layout=AS.DEFAULT_LAYOUT):
    from upkie_amd.privileged import PrivilegedObservation

    N, D, A = num_envs, layout.D, layout.A
    dev = torch.device(DEV)
    randomized = [1 if k in layout.links else 0 for k in range(AS.PRIVILEGED_MAX_LINKS)]
    env = types.SimpleNamespace(num_envs=N, device=dev, model=types.SimpleNamespace(num_links=AS.PRIVILEGED_MAX_LINKS, link_randomized=randomized))
    events = types.SimpleNamespace(num_envs=N, force=torch.zeros(1, 3, N, device=dev), link_scale=torch.ones(AS.PRIVILEGED_MAX_LINKS, N, device=dev))
    pipeline = types.SimpleNamespace(num_envs=N, obs_dim=D, act_dim=A, command=torch.zeros(N, A, device=dev))
    stage = PrivilegedObservation(env, events=events, pipeline=pipeline, include=layout.include)
    assert stage.dim == AS.layout_dim(layout) and ("link_scale" not in layout.include or stage.links.tolist() == list(layout.links))
    inputs = {"next_obs": torch.zeros(N, D, device=dev), "final_obs": torch.zeros(N, D, device=dev),
              "terminated": torch.zeros(N, dtype=torch.uint8, device=dev), "truncated": torch.zeros(N, dtype=torch.uint8, device=dev)}
    return stage, events, pipeline, inputs


def _feed(call, events, pipeline, inputs):
    events.force[0].copy_(torch.from_numpy(call["force"]))
    events.link_scale.copy_(torch.from_numpy(call["link_scale"]))
    pipeline.command.copy_(torch.from_numpy(call["command"]))
    for name, t in inputs.items():
        t.copy_(torch.from_numpy(call[name]))


@pytest.mark.parametrize("num_envs", AS.PRIVILEGED_SIZES)
def test_the_privileged_stage_is_its_twin_after_every_call(num_envs):
    calls = AS.privileged_calls(num_envs)
    want = AS.run_privileged_twin(num_envs, calls)
    results = {}
    for graphed in (False, True):
        stage, events, pipeline, inputs = _stage(num_envs)
        _feed(calls[0], events, pipeline, inputs)
        stage.reset(inputs["next_obs"])
        step = lambda: stage.step(inputs["next_obs"], inputs["terminated"], inputs["truncated"], final_obs=inputs["final_obs"])  # noqa: E731
        if graphed:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            step = graph.replay
        got = [(stage.observation.cpu().numpy().copy(), None)]
        for call in calls[1:]:
            _feed(call, events, pipeline, inputs)
            step()
            torch.cuda.synchronize()
            got.append((stage.observation.cpu().numpy().copy(), stage.final_observation.cpu().numpy().copy()))
        results[graphed] = got
    view = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    for k, ((row, final), (want_row, want_final)) in enumerate(zip(results[False], want)):
        assert np.array_equal(view(row), view(want_row)), k
        assert final is None or np.array_equal(view(final), view(want_final)), k
    for k, ((row, final), (g_row, g_final)) in enumerate(zip(results[False], results[True])):
        assert np.array_equal(view(row), view(g_row)) and (final is None or np.array_equal(view(final), view(g_final))), k


LAYOUT_CASES, LAYOUT_IDS = AS.layout_cases()
GRAPHED_LAYOUT = ("27-columns", 129)  # replayed from graphs as well: seven staging passes, a last block of one env


@pytest.mark.parametrize("layout,num_envs", LAYOUT_CASES, ids=LAYOUT_IDS)
def test_the_privileged_stage_at_its_layouts(layout, num_envs):
    """Every layout of tests/asymmetric_shapes.py besides the default, at its sizes, through `SCRIPT`: steps with and
    without final_obs and end flags, resets under a mixed mask, a zero mask and none. Both buffers are the twin's bits after
    every call (a masked reset's other rows and every terminal row keep theirs); one case also replays each kind of call
    from a graph of its own."""
    N = num_envs
    calls = AS.layout_calls(layout, N)
    want = AS.run_privileged_twin(N, calls, layout=layout)
    view = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    results = {}
    for graphed in (False, True) if (layout.name, N) == GRAPHED_LAYOUT else (False,):
        stage, events, pipeline, inputs = _stage(N, layout)
        mask = torch.zeros(N, dtype=torch.uint8, device=DEV)
        _feed(calls[0], events, pipeline, inputs)
        stage.reset(inputs["next_obs"])
        flags = (inputs["terminated"], inputs["truncated"])
        ops = {"step": lambda: stage.step(inputs["next_obs"], *flags, final_obs=inputs["final_obs"]),
               "step_no_final": lambda: stage.step(inputs["next_obs"], *flags),
               "step_no_flags": lambda: stage.step(inputs["next_obs"], final_obs=inputs["final_obs"]),
               "reset_mixed": lambda: stage.reset(inputs["next_obs"], mask),
               "reset_zero": lambda: stage.reset(inputs["next_obs"], mask),
               "reset_all": lambda: stage.reset(inputs["next_obs"])}
        if graphed:
            torch.cuda.synchronize()
            for op in list(ops):
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    ops[op]()
                ops[op] = graph.replay
        got = [(stage.observation.cpu().numpy().copy(), None)]
        for call in calls[1:]:
            _feed(call, events, pipeline, inputs)
            if call["mask"] is not None:
                mask.copy_(torch.from_numpy(call["mask"]))
            ops[call["op"]]()
            torch.cuda.synchronize()
            got.append((stage.observation.cpu().numpy().copy(), stage.final_observation.cpu().numpy().copy()))
        results[graphed] = got
    assert np.array_equal(view(results[False][0][0]), view(want[0][0])), "the first rows"
    for graphed, got in results.items():
        for k, ((row, final), (want_row, want_final)) in enumerate(zip(got[1:], want[1:]), start=1):
            where = (k, calls[k]["op"], "graphed" if graphed else "eager")
            assert np.array_equal(view(row), view(want_row)), where
            assert np.array_equal(view(final), view(want_final)), where


# ---------------------------------------------------------------- 6. Ppo with a privileged critic
B, STEPS = 64, 8
EVENTS = dict(push_prob=0.1, push_norm=(5.0, 20.0), push_steps=(1, 3), inertia_variation=0.2)


def _make(privileged=True, **kw):
    from upkie_amd.events import EpisodeEvents
    from upkie_amd.pipeline import AgentPipeline
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.ppo import Ppo
    from upkie_amd.privileged import PrivilegedObservation

    torch.manual_seed(0)
    env = pendulum(B, 5, seed=0)
    dev = env.device
    events = EpisodeEvents(env, **EVENTS)
    pipeline = AgentPipeline(B, 4, [-1.0], [1.0], dt=1.0 / 200.0, stack=2, observation_noise=[0.01] * 4, action_lag=0.05, seed=5, device=dev)
    rows = PrivilegedObservation(env, events=events, pipeline=pipeline) if privileged else None
    actor = tower(pipeline.stacked_dim, 1).to(dev)
    critic = tower(rows.dim if privileged else pipeline.stacked_dim, 1).to(dev)
    policy = MlpActorCritic.from_modules(actor, critic, nn.Parameter(torch.zeros(1, device=dev)), action_low=[-1.0], action_high=[1.0], seed=0)
    args = dict(n_steps=STEPS, n_epochs=2, batch_size=B * STEPS // 2, seed=0, reward_fn=pitch_reward)
    model = Ppo(env, policy, events=events, pipeline=pipeline, critic_observation=rows, **args, **kw)
    return env, policy, model, args


def test_ppo_with_a_privileged_critic_graphed_eager_and_resumed(tmp_path):
    from upkie_amd.ppo import Ppo

    env, policy, model, args = _make(graph=True)
    assert policy.asymmetric and policy.critic_obs_dim == model.critic_observation.dim == 4 + 1 + 3 + len(model.critic_observation.links)
    with env:
        model.learn(2 * B * STEPS)
        graphed = snapshot(model, ("buffer.critic_observations",))
    env, policy, model, _ = _make(graph=False)
    with env:
        model._setup()
        model._slot = model.n_steps - 1  # (a graphed Ppo runs one real rollout step into the last slot before it captures)
        model._rollout_step()
        model.learn(2 * B * STEPS)
        eager = snapshot(model, ("buffer.critic_observations",))
    keys = ("critic_observation.observation", "critic_observation.final_observation", "critic_normalizer", "packed", "m", "v", "events.force")
    assert all(k in graphed[0] for k in keys)
    for k in graphed[0]:
        assert same(graphed[0][k], eager[0][k]), k
    assert same(graphed[1], eager[1]) and len(graphed[1]) == 2
    assert float(graphed[0]["critic_normalizer"]["obs_count"]) > 2 * STEPS * B and graphed[0]["events.pushes"].sum() > 0

    path = str(tmp_path / "ppo.pt")
    env, policy, model, _ = _make(graph=True)
    with env:
        model.learn(2 * B * STEPS, callback=lambda m, rec: m.iterations < 1)
        assert model.iterations == 1
        model.save(path)
    env, policy, fresh, args = _make(graph=True)
    with env:
        resumed = Ppo.load(path, env, policy, events=fresh.events, pipeline=fresh.pipeline, critic_observation=fresh.critic_observation, **args)
        resumed.learn(B * STEPS, reset_num_timesteps=False)
        end = snapshot(resumed, ("buffer.critic_observations",))
    for k in graphed[0]:
        assert same(graphed[0][k], end[0][k]), k
    assert same(graphed[1][1:], end[1])


def test_the_buffers_rows_are_the_twins_and_evaluation_ignores_the_critic():
    """Eager and without normalisation the buffer holds the raw rows: slot t is the twin's row before step t, fed the env's
    recorded outputs and the stages' buffers as they stood after `events.step`. Then the trained policy is evaluated, and
    so is a symmetric policy built from the same actor: the critic never runs, the results are equal."""
    from upkie_amd.evaluation import evaluate_policy
    from upkie_amd.policies import MlpActorCritic

    env, policy, model, _ = _make(graph=False, normalize=False)
    with env:
        model._setup()
        rows, events, pipeline = model.critic_observation, model.events, model.pipeline
        grab = lambda: {"command": pipeline.command.cpu().numpy().copy(), "force": events.force[0].cpu().numpy().copy(),  # noqa: E731
                        "link_scale": events.link_scale.cpu().numpy().copy()}
        links = rows.links.tolist()
        twin = AR.PrivilegedTwin(B, 4, 1, links)
        first = grab()
        twin.reset(model._agent.raw_observation.cpu().numpy(), first["command"], first["force"], first["link_scale"])
        assert np.array_equal(twin.observation, rows.observation.cpu().numpy()), "the first rows"
        recorded, inner = [], rows.step

        def recording_step(next_obs, terminated, truncated, final_obs=None):
            call = dict(grab(), next_obs=next_obs.cpu().numpy().copy(), final_obs=final_obs.cpu().numpy().copy(),
                        terminated=terminated.cpu().numpy().astype(np.uint8), truncated=truncated.cpu().numpy().astype(np.uint8))
            recorded.append(call)
            return inner(next_obs, terminated, truncated, final_obs=final_obs)

        rows.step = recording_step
        model.learn(B * STEPS)
        torch.cuda.synchronize()
        assert len(recorded) == STEPS
        got = model.buffer.critic_observations.cpu().numpy()
        ended = 0
        for t, c in enumerate(recorded):
            assert np.array_equal(got[t], twin.observation), t
            twin.step(c["next_obs"], c["final_obs"], c["command"], c["force"], c["link_scale"], c["terminated"], c["truncated"])
            ended += int((c["terminated"] | c["truncated"]).sum())
        assert np.array_equal(twin.observation, rows.observation.cpu().numpy()) and np.array_equal(twin.final_observation, rows.final_observation.cpu().numpy())
        assert ended > 0 and np.abs(got[:, :, rows.segment("push_force")]).sum() > 0 and np.ptp(got[:, :, rows.segment("link_scale")]) > 0

        actor = model.policy._modules[0]
        symmetric = MlpActorCritic.from_modules(actor, tower(pipeline.stacked_dim, 1).to(env.device), model.policy._modules[2], action_low=[-1.0],
                                                action_high=[1.0], seed=0)
        results = []
        for pol in (policy, symmetric):
            with pendulum(32, 6, seed=9) as eval_env:
                from upkie_amd.pipeline import AgentPipeline

                eval_pipe = AgentPipeline(32, 4, [-1.0], [1.0], dt=1.0 / 200.0, stack=2, observation_noise=[0.01] * 4, action_lag=0.05, seed=5,
                                          device=eval_env.device)
                results.append(evaluate_policy(pol, eval_env, n_eval_episodes=48, reward_fn=pitch_reward, seed=9, pipeline=eval_pipe, chunk=4,
                                               return_episode_rewards=True))
        assert results[0] == results[1] and len(results[0][0]) == 48


def test_the_privileged_example_runs():
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EXAMPLE_STEPS="16", EXAMPLE_ENVS="64")
    result = subprocess.run([sys.executable, os.path.join(root, "examples", "ppo_learn_privileged.py")], capture_output=True, text=True, timeout=600,
                            env=env, cwd=os.path.join(root, "examples"))
    assert result.returncode == 0, result.stderr[-3000:]
    lines = [ln for ln in result.stdout.splitlines() if ln.startswith("iteration")]
    assert len(lines) == 3 and all("train/loss" in ln for ln in lines), result.stdout
    assert "the actor reads 40 words, the critic 20" in result.stdout and "evaluate_policy, pushed, no critic:" in result.stdout
