"""Policy distillation without a GPU: the fp64 twins of tests/distill_reference.py against torch autograd, the header
against the ctypes bindings, every refusal by name, the mix twin's invariances, that the GPU tests' inputs tell the likely
one-line mistakes from the feature, and the driver's call order through `AgentStep` on the CPU oracle env."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import distill_reference as R
from tests import mlp_shapes as S
from upkie_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_BOUND = S.DEFAULT_BOUNDS["grad"]
ROWS = [pytest.param(i, r, id=S.row_id(r)) for i, r in enumerate(S.MATRIX)]


# ---------------------------------------------------------------- the gradient twin
@pytest.mark.parametrize("index", [0, 1, 4, 8, 12])
def test_the_gradient_twin_is_torch_autograd_of_mse_loss(index):
    """fp64 autograd of the literal ``mse_loss(actor(x), label)`` on the row's modules, normalising rows included."""
    row = S.MATRIX[index]
    shape, sources, obs, labels = R.gradient_case(index, row)
    obs, labels = obs[:200], labels[:200]
    actor, _ = S.row_modules(row)
    actor = actor.double()
    x = torch.as_tensor(R.normalized(shape, sources, obs))
    loss = torch.nn.functional.mse_loss(actor(x), torch.as_tensor(labels, dtype=torch.float64))
    params = [p for m in actor if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]
    want = torch.autograd.grad(loss, params)
    got_loss, grads, norm = R.minibatch(shape, sources, obs, labels)
    assert got_loss == pytest.approx(float(loss.detach()), rel=1e-12)
    sl = R.actor_slice(shape)
    assert len(grads[sl]) == len(want)
    for g, w in zip(grads[sl], want):
        np.testing.assert_allclose(g.reshape(w.shape), w.numpy(), rtol=1e-12, atol=1e-300 + 1e-12 * float(w.abs().max()))
    for k, g in enumerate(grads):
        if not sl.start <= k < sl.stop:
            assert not np.any(g), "log_std and the critic get no gradient"
    assert norm == pytest.approx(float(torch.sqrt(sum((w * w).sum() for w in want))), rel=1e-12)


def test_the_update_twin_is_torch_clip_and_adam():
    index, row = 4, S.MATRIX[4]
    shape, sources, obs, labels = R.gradient_case(index, row)
    obs, labels = obs[:300], labels[:300]
    actor, _ = S.row_modules(row)
    actor = actor.double()
    params = [p for m in actor if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]
    opt = torch.optim.Adam(params, lr=1e-3, eps=1e-5)
    rng = np.random.default_rng(0)
    perms = [rng.permutation(300) for _ in range(2)]
    x, y = torch.as_tensor(R.normalized(shape, sources, obs)), torch.as_tensor(labels, dtype=torch.float64)
    for perm in perms:
        for start in range(0, 300, 128):
            i = torch.as_tensor(perm[start:start + 128])
            opt.zero_grad()
            torch.nn.functional.mse_loss(actor(x[i]), y[i]).backward()
            torch.nn.utils.clip_grad_norm_(params, 0.05)
            opt.step()
    after, (m, v, t), stats, _ = R.update(shape, sources, obs, labels, perms, 128, lr=1e-3, max_grad_norm=0.05)
    assert t == 6 and stats.shape == (2, 3, 3) and np.all(stats[:, :, 2] < 1.0), "the clip bites"
    for got, want in zip(R.trainable(shape, after)[R.actor_slice(shape)], params):
        np.testing.assert_allclose(got.reshape(want.shape), want.detach().numpy(), rtol=1e-9, atol=1e-12)
    before = R.trainable(shape, sources)
    for k, (a, b) in enumerate(zip(R.trainable(shape, after), before)):
        if not R.actor_slice(shape).start <= k < R.actor_slice(shape).stop:
            assert np.array_equal(a, b) and not np.any(m[k]) and not np.any(v[k])


# ---------------------------------------------------------------- header, bindings
def _header():
    with open(os.path.join(ROOT, "include", "upkie_hip.h")) as f:
        return f.read()


def test_header_constants_and_signatures_match_the_bindings():
    text = _header()
    assert int(re.search(r"UPKIE_DISTILL_STATS = (\d+)", text).group(1)) == abi.DISTILL_STATS == len(abi.DISTILL_STAT_NAMES)
    with open(os.path.join(ROOT, "upkie_amd", "csrc", "random.hpp")) as f:
        assert int(re.search(r"STREAM_DISTILL = (\d+)", f.read()).group(1)) == abi.STREAM_DISTILL == R.STREAM_DISTILL
    assert f"{abi.STREAM_DISTILL} << 24" in text, "the header states the mix's stream tag"
    table = {name: (restype, argtypes) for name, restype, argtypes, _ in lib._ABI}
    kinds = {"int32_t": C.c_int32, "double": C.c_double}
    for name in ("upkie_distill_workspace_bytes", "upkie_distill_minibatch_update", "upkie_sim_distill_mix"):
        ret, args = re.search(r"(int64_t|int) " + name + r"\(([^;]*)\);", text).groups()
        args = [" ".join(a.split()) for a in args.split(",")]
        want = []
        for a in args:
            if "*" in a:
                want.append("shape" if "UpkieMlpShape" in a else C.c_void_p)
            else:
                want.append(kinds[a.rsplit(" ", 1)[0]])
        restype, argtypes = table[name]
        assert restype is (C.c_int64 if ret == "int64_t" else C.c_int)
        got = ["shape" if t is C.POINTER(abi.UpkieMlpShape) else t for t in argtypes]
        if name != "upkie_distill_workspace_bytes":
            assert args[-1] == "void* stream"
        assert got == want, name
    assert "upkie_distill_minibatch_update" in lib.EXPORTED_SYMBOLS and "upkie_sim_distill_mix" in lib.EXPORTED_SYMBOLS


def _shape(critic=True, D=4, A=2):
    from upkie_amd.policies import mlp_shape

    return mlp_shape(S.dims(D, [16], A), S.dims(D, [16], 1) if critic else [], "tanh")


def _last_error(handle):
    return handle.upkie_sim_last_error(None).decode()


def test_the_library_refuses_by_name_without_a_device():
    handle = lib.load()
    good, bare = _shape(), _shape(critic=False)
    assert handle.upkie_distill_workspace_bytes(C.byref(bare), 64) == abi.ERR_INVALID_ARGUMENT
    assert "distillation needs a student with a critic" in _last_error(handle)
    assert handle.upkie_distill_workspace_bytes(C.byref(good), 0) == abi.ERR_INVALID_ARGUMENT and "max_minibatch" in _last_error(handle)
    assert handle.upkie_distill_workspace_bytes(C.byref(good), 64) > 0
    one = (C.c_double * 2)()
    p = C.addressof(one)
    args = [C.byref(good), 64, 0, 64, 64, p, p, p, p, p, p, p, 1.0, 0.9, 0.999, 1e-5, 0, p, p, None]
    for change, message in (({0: C.byref(bare)}, "needs a student with a critic"), ({3: 65}, "minibatch out of range"), ({2: 1}, "minibatch out of range"),
                            ({7: None}, "null argument"), ({12: 0.0}, "max_grad_norm"), ({13: 1.0}, "adam betas"), ({11: p + 4}, "8-byte aligned")):
        a = list(args)
        for k, v in change.items():
            a[k] = v
        assert handle.upkie_distill_minibatch_update(*a) == abi.ERR_INVALID_ARGUMENT, message
        assert message in _last_error(handle), (message, _last_error(handle))
    # an asymmetric shape is taken: the critic's rows are not needed
    from upkie_amd.policies import asymmetric_shape

    asym = asymmetric_shape(good, 9)
    assert handle.upkie_distill_workspace_bytes(C.byref(asym), 64) > 0
    # the mix: every refusal before any device use (a NULL handle included)
    assert handle.upkie_sim_distill_mix(None, 0, p, p, p, p, p, p, p, p, None) == abi.ERR_INVALID_ARGUMENT and "act_dim" in _last_error(handle)
    assert handle.upkie_sim_distill_mix(None, 65, p, p, p, p, p, p, p, p, None) == abi.ERR_INVALID_ARGUMENT
    assert handle.upkie_sim_distill_mix(None, 2, p, p, p, p, p, p, p, p, None) == abi.ERR_INVALID_ARGUMENT and "null argument" in _last_error(handle)


def _student_stub(critic=True):
    """An `MlpActorCritic` object with a shape and nothing else (building a real one needs the device)."""
    from upkie_amd.policies import MlpActorCritic

    stub = MlpActorCritic.__new__(MlpActorCritic)
    stub.shape = _shape(critic)
    return stub


def test_the_trainer_refuses_by_name():
    from upkie_amd.distill import DistillTrainer, beta_threshold

    with pytest.raises(TypeError, match="trains an MlpActorCritic"):
        DistillTrainer(object())
    with pytest.raises(ValueError, match="needs a student with a critic"):
        DistillTrainer(_student_stub(critic=False))
    with pytest.raises(ValueError, match="process_group is not supported"):
        DistillTrainer(_student_stub(), process_group=object())
    with pytest.raises(ValueError, match="n_epochs and batch_size"):
        DistillTrainer(_student_stub(), n_epochs=0)
    # the label's shape, checked before any launch
    tr = DistillTrainer.__new__(DistillTrainer)
    tr.policy, tr.device, tr.obs_normalized = _student_stub(), torch.device("cpu"), True
    obs = torch.zeros(3, 5, 4)
    assert tr._check(obs, torch.zeros(3, 5, 2)) == 15
    for labels in (torch.zeros(3, 5, 3), torch.zeros(3, 4, 2), torch.zeros(15, 2)):
        with pytest.raises(ValueError, match=r"labels must be \[3, 5, 2\]"):
            tr._check(obs, labels)
    with pytest.raises(ValueError, match="observations hold 5 words per sample, the student reads 4"):
        tr._check(torch.zeros(3, 5, 5), torch.zeros(3, 5, 2))
    with pytest.raises(ValueError, match="contiguous float32"):
        tr._check(obs.double(), torch.zeros(3, 5, 2))
    assert [beta_threshold(b) for b in (0.0, 0.5, 1.0)] == [0, 1 << 23, 1 << 24] == [R.threshold(b) for b in (0.0, 0.5, 1.0)]
    with pytest.raises(ValueError, match=r"beta must be in \[0, 1\]"):
        beta_threshold(1.5)


# ---------------------------------------------------------------- the driver on doubles
from tests.agent_step_doubles import A, D, N, T, Calls, Env, Episodes, Normalizer, Pipeline, Policy, filler, saved_parts, stage  # noqa: E402


class _Student(Policy):
    """tests/agent_step_doubles.py's policy with the actor-only call the driver makes."""

    def __init__(self, obs_dim, calls):
        super().__init__(obs_dim, calls)
        self.action_low, self.action_high = torch.full((A,), -1.0), torch.full((A,), 1.0)

    def act_actor(self, obs, deterministic=False, out=None):
        self.calls.add("act_actor", obs=obs, out=out, deterministic=deterministic, seen=obs.clone())
        out["action"].fill_(0.5)
        if "norm_obs" in out:
            out["norm_obs"].copy_(obs).mul_(2.0)


class _Teacher:
    obs_dim, act_dim = D, A

    def __init__(self, calls):
        self.calls = calls

    def __call__(self, obs, out):
        self.calls.add("teacher", obs=obs, out=out, seen=obs.clone())
        out.fill_(-0.25)


class _Mix:
    def __init__(self, calls):
        self.calls, self.applied = calls, torch.zeros(N, A)

    def step(self, label, student_action, drove):
        self.calls.add("mix", label=label, student_action=student_action, drove=drove)
        self.applied.copy_(label)
        drove.fill_(1)
        return self.applied


class _Privileged:
    dim, num_envs = 7, N

    def __init__(self, calls):
        self.calls, self.observation = calls, torch.zeros(N, 7)

    def step(self, next_obs, terminated, truncated, final_obs=None):
        self.calls.add("privileged", next_obs=next_obs, terminated=terminated, truncated=truncated, final_obs=final_obs)


def _oracle_env(calls):
    import upkie_amd.envs as envs
    from tests.fake_sim import oracle_sim_factory
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    inner = envs.make("Upkie-HIP-Pendulum-Vec", num_envs=N, frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=4,
                      sim_factory=oracle_sim_factory)
    return inner, Env(inner, calls)


def _model(env, calls, pipeline, normalizer, privileged):
    """A `Distillation` set up by hand as `_setup` would, with the doubles in the stages' places."""
    from upkie_amd.distill import Distillation

    pipe = Pipeline(calls) if pipeline else None
    words = pipe.stacked_dim if pipeline else D
    teacher = _Teacher(calls)
    priv = _Privileged(calls) if privileged else None
    if privileged:
        teacher.obs_dim = 7
    model = Distillation(env, _Student(words, calls), teacher, teacher_observation=priv if privileged else "raw", n_steps=T, pipeline=pipe,
                         normalize=normalizer, graph=False)
    model.normalizer = Normalizer(calls) if normalizer else None
    model.episodes, model.mix = Episodes(calls), _Mix(calls)
    model.observations, model.labels = torch.zeros(T, N, words), torch.zeros(T, N, A)
    model.drove = torch.zeros(T, N, dtype=torch.uint8)
    model._action, model._norm_reward, model._starts = torch.zeros(N, A), torch.zeros(N), torch.ones(N, dtype=torch.uint8)
    model._slot = 2
    return model


@pytest.mark.parametrize("pipeline,normalizer,privileged", [(False, False, False), (False, True, False), (True, True, False), (True, False, True),
                                                             (False, True, True)])
def test_a_rollout_step_calls_the_stages_in_order_with_the_same_tensors(pipeline, normalizer, privileged):
    calls = Calls()
    inner, env = _oracle_env(calls)
    with inner:
        model = _model(env, calls, pipeline, normalizer, privileged)
        reset = inner.reset(seed=0)
        model._agent.raw_observation = first = reset[0] if isinstance(reset, tuple) else reset
        pipe = model.pipeline
        model.collect_rollouts()
    step = (["act_actor", "teacher", "mix"] + (["shape_action"] if pipeline else []) + ["env.step"] + (["privileged"] if privileged else [])
            + ["episodes"] + (["observe"] if pipeline else []) + (["normalizer"] if normalizer else []))
    assert calls.names == step * T
    assert model._slot == 2 and model.num_timesteps == T * N
    args, raw = calls.args, first
    for k in range(T):
        t = (2 + k) % T
        act = args["act_actor"][k]
        assert act["obs"] is (pipe.observation if pipeline else raw) and act["out"]["action"] is model._action and act["deterministic"] is False
        if normalizer:
            assert act["out"]["norm_obs"].data_ptr() == model.observations[t].data_ptr()
        else:
            assert set(act["out"]) == {"action"} and torch.equal(model.observations[t], act["seen"])
        # the teacher's row at the same instant, its label straight into the slot
        seen = args["teacher"][k]
        assert seen["obs"] is (model.teacher_observation.observation if privileged else raw)
        assert seen["out"].data_ptr() == model.labels[t].data_ptr()
        mix = args["mix"][k]
        assert mix["label"].data_ptr() == model.labels[t].data_ptr() and mix["student_action"] is model._action
        assert mix["drove"].data_ptr() == model.drove[t].data_ptr()
        stepped = args["env.step"][k]
        if pipeline:
            assert args["shape_action"][k]["env_action"] is model.mix.applied
        assert stepped["action"] is (pipe.command if pipeline else model.mix.applied)
        next_obs, env_reward, terminated, truncated, info = stepped["out"]
        same = dict(terminated=terminated, truncated=truncated)
        if privileged:
            p = args["privileged"][k]
            assert p["next_obs"] is next_obs and p["final_obs"] is info["final_obs"] and all(p[n] is x for n, x in same.items())
        assert args["episodes"][k]["reward"] is env_reward and all(args["episodes"][k][n] is x for n, x in same.items())
        if pipeline:
            o = args["observe"][k]
            assert o["next_obs"] is next_obs and o["final_obs"] is info["final_obs"]
        if normalizer:
            n_ = args["normalizer"][k]
            assert n_["obs"] is (pipe.observation if pipeline else next_obs) and n_["reward"] is env_reward
        raw = next_obs
    assert torch.all(model.labels == -0.25) and torch.all(model.drove == 1)


def test_the_driver_refuses_by_name():
    from upkie_amd.distill import Distillation
    from upkie_amd.policies import LinearPolicy

    calls = Calls()
    env = type("E", (), {"num_envs": N})()
    student = _Student(D, calls)
    with pytest.raises(ValueError, match="process_group is not supported"):
        Distillation(env, student, _Teacher(calls), process_group=object())
    wide = LinearPolicy(torch.zeros(7, A), device="cpu")
    with pytest.raises(ValueError, match="teacher_observation has 4 words, the teacher's obs_dim is 7"):
        Distillation(env, student, wide)
    with pytest.raises(ValueError, match="teacher_observation has 7 words, the teacher's obs_dim is 4"):
        Distillation(env, student, _Teacher(calls), teacher_observation=_Privileged(calls))
    with pytest.raises(ValueError, match="the teacher gives 3 actions, the student's act_dim is 1"):
        Distillation(env, student, LinearPolicy(torch.zeros(D, 3), device="cpu"))
    with pytest.raises(ValueError, match="teacher_observation must be 'raw' or a PrivilegedObservation"):
        Distillation(env, student, _Teacher(calls), teacher_observation="privileged")
    with pytest.raises(TypeError, match="teacher must be"):
        Distillation(env, student, 3.0)
    with pytest.raises(ValueError, match=r"beta must be in \[0, 1\]"):
        Distillation(env, student, _Teacher(calls), beta=2.0)
    # with a pipeline the raw row is the pipeline's input, not the student's stack
    pipe = Pipeline(calls)
    with pytest.raises(ValueError, match=f"teacher_observation has {D} words, the teacher's obs_dim is {pipe.stacked_dim}"):
        teacher = _Teacher(calls)
        teacher.obs_dim = pipe.stacked_dim
        Distillation(env, _Student(pipe.stacked_dim, calls), teacher, pipeline=pipe)


def test_ppo_refuses_a_hand_over_it_cannot_continue():
    """`Ppo` keeps the live normaliser of a policy that has been called (a distilled student); what it cannot keep it
    refuses by name, before it builds anything: another env size, another gamma, an asymmetric continuation."""
    import types

    from upkie_amd.ppo import Ppo

    calls = Calls()
    env = types.SimpleNamespace(num_envs=N, device="cpu")

    def student(num_envs=N, gamma=0.99):
        pol = _Student(D, calls)
        pol._normalizer, pol._out = types.SimpleNamespace(num_envs=num_envs, gamma=gamma), {"n": N}
        return pol

    with pytest.raises(ValueError, match=f"the policy's normaliser serves {N + 1} envs at gamma 0.99, this run has {N} at 0.99"):
        Ppo(env, student(num_envs=N + 1), n_steps=T, graph=False)._setup()
    with pytest.raises(ValueError, match=f"the policy's normaliser serves {N} envs at gamma 0.9, this run has {N} at 0.99"):
        Ppo(env, student(gamma=0.9), n_steps=T, graph=False)._setup()
    asym = student()
    asym.asymmetric, asym.critic_obs_dim = True, _Privileged.dim
    with pytest.raises(ValueError, match="taken over for symmetric training only"):
        Ppo(env, asym, n_steps=T, graph=False, critic_observation=_Privileged(calls))._setup()


def test_the_twins_launch_geometry_is_the_librarys():
    """`distill_reference.actor_plan` (what the GPU test reads the waves per block and the grid cap from) gives the
    workspace size the library gives on every row of the matrix; and the matrix has a row whose
    chunks exceed the ACTOR span's grid cap, and rows of 1, 2, 3 and 4 waves."""
    from tests import ppo_reference as PR

    handle = lib.load()
    above, waves = 0, set()
    for row in S.MATRIX:
        shape = S.shape_of(row)
        plan = R.actor_plan(shape)
        for n in (1, 100, S.T * row.N, 131072):
            assert handle.upkie_distill_workspace_bytes(C.byref(shape), n) == PR.workspace_bytes(plan, n), (S.row_id(row), n)
        assert plan["train_words"] < PR.plan(shape)["train_words"] and plan["grid_cap"] >= PR.plan(shape)["grid_cap"]
        above += PR.chunks(plan, S.T * row.N) > plan["grid_cap"]
        waves.add(plan["nw"])
    assert above >= 1 and waves == {1, 2, 3, 4}


# ---------------------------------------------------------------- Distillation.save / Distillation.load: what the file holds
def _saved_distillation():
    from upkie_amd.distill import DaggerMix, Distillation, DistillTrainer
    from upkie_amd.episodes import EpisodeStatistics

    class Saved(Distillation):
        """`Distillation` whose stages are host stand-ins (as tests/test_ppo_learn.py's `_SavedPpo`)."""

        def _setup(self):
            if self.observations is not None:
                return
            scale = self.env.scale
            f = filler(range(1, 100), scale)
            self.observations, self.device, self.normalizer = object(), torch.device("cpu"), None
            self.trainer = stage(DistillTrainer, m=f(6), v=f(6), scalars=f(2, dtype=torch.float64), generator=torch.Generator(), _lr=1e-3 * scale,
                                 sync_modules=lambda: None)
            self.trainer.generator.manual_seed(5 * scale)
            self.episodes = stage(EpisodeStatistics, ep_return=f(2, dtype=torch.float64), ep_length=f(2, dtype=torch.int32),
                                  ring_return=f(3, dtype=torch.float64), ring_length=f(3, dtype=torch.int32), counters=f(3, dtype=torch.int64),
                                  means=f(2, dtype=torch.float64))
            self.mix = stage(DaggerMix, calls=f(2, dtype=torch.int32), threshold=f(1, dtype=torch.int32))
            self._starts, self._agent.raw_observation = f(2, dtype=torch.uint8), f(2, 4)

    return Saved


class _RawTeacher:
    act_dim = A

    def __call__(self, obs, out):
        out.zero_()


DISTILL_TENSORS = (["packed", "calls", "m", "v", "scalars", "mix.calls", "mix.threshold"]
                   + ["episodes." + k for k in ("ep_return", "ep_length", "ring_return", "ring_length", "counters", "means")]
                   + ["env." + k for k in ("state", "reward", "terminated", "truncated", "final_obs", "observation")])
EXTRA_STAGES = ("events", "targets", "teacher_observation")


@pytest.mark.parametrize("pipeline,reward,stages", [(False, False, ()), (True, False, ()), (False, True, ()), (False, True, EXTRA_STAGES)],
                         ids=("plain", "pipeline", "reward", "every-stage"))
def test_save_writes_these_names_and_load_puts_them_back(tmp_path, monkeypatch, pipeline, reward, stages):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: None)
    Saved, path = _saved_distillation(), str(tmp_path / "distill.pt")
    env, student, kwargs = saved_parts(1, pipeline, reward, stages)
    model = Saved(env, student, _RawTeacher(), n_steps=4, beta=0.25, **kwargs)
    model._setup()
    model.num_timesteps, model.iterations, model.total_timesteps, model.progress_remaining = 24, 3, 80, 0.7
    model.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(sd) == ["counters", "generator", "normalizer", "sizes", "tensors"]
    names = DISTILL_TENSORS + [f"{s}.{k}" for s in kwargs for k in kwargs[s].state_tensors()]
    assert sorted(sd["tensors"]) == sorted(names) and "starts" not in sd["tensors"]
    for s, given in (("pipeline", pipeline), ("reward", reward), ("events", stages), ("targets", stages), ("teacher_observation", stages)):
        assert any(k.startswith(s + ".") for k in sd["tensors"]) == bool(given), s
    assert sd["counters"] == {"num_timesteps": 24, "iterations": 3, "total_timesteps": 80, "progress_remaining": 0.7, "policy_seed": 7, "beta": 0.25,
                              "lr": 1e-3}
    assert sd["sizes"] == {"n_envs": 2, "n_steps": 4} and sd["normalizer"] is None
    # every name holds the tensor of the stage that owns it
    tr, ep = model.trainer, model.episodes
    owners = {"packed": student.packed, "calls": student.calls, "m": tr.m, "v": tr.v, "scalars": tr.scalars, "mix.calls": model.mix.calls,
              "mix.threshold": model.mix.threshold, "env.state": env.sim.state, "env.reward": env.sim.reward, "env.terminated": env.sim.terminated,
              "env.truncated": env.sim.truncated, "env.observation": model._agent.raw_observation, "env.final_obs": env._final_obs}
    owners.update({f"episodes.{k}": v for k, v in ep.state_tensors().items()})
    owners.update({f"{s}.{k}": v for s in kwargs for k, v in kwargs[s].state_tensors().items()})
    assert owners.keys() == sd["tensors"].keys() and all(torch.equal(sd["tensors"][k], v) and sd["tensors"][k].dtype == v.dtype for k, v in owners.items())
    # into fresh objects holding other numbers
    env2, student2, kwargs2 = saved_parts(2, pipeline, reward, stages)
    loaded = Saved.load(path, env2, student2, _RawTeacher(), n_steps=4, beta=0.5, **kwargs2)
    assert all(torch.equal(sd["tensors"][k], v) for k, v in loaded._state_tensors().items()) and loaded._state_tensors().keys() == owners.keys()
    assert torch.equal(student2.packed, student.packed) and torch.equal(loaded.episodes.counters, ep.counters) and student2.seed == 7
    assert torch.equal(loaded.mix.threshold, model.mix.threshold) and torch.equal(loaded.trainer.scalars, tr.scalars)
    assert torch.equal(loaded.trainer.generator.get_state(), tr.generator.get_state())
    assert (loaded.num_timesteps, loaded.iterations, loaded.total_timesteps, loaded.progress_remaining) == (24, 3, 80, 0.7)
    assert (loaded._beta, loaded.trainer._lr) == (0.25, 1e-3)
    if not reward:  # a file without a stage's tensors does not load into a run with that stage: refused by name
        env3, student3, kwargs3 = saved_parts(2, pipeline, True)
        with pytest.raises(ValueError, match="the file has no reward.prev_action"):
            Saved.load(path, env3, student3, _RawTeacher(), n_steps=4, **kwargs3)
    if not stages and not pipeline:
        env3, student3, kwargs3 = saved_parts(2, pipeline, reward, ("events",))
        with pytest.raises(ValueError, match="the file has no events.calls"):
            Saved.load(path, env3, student3, _RawTeacher(), n_steps=4, **kwargs3)
    with pytest.raises(ValueError, match=r"the file holds a run of \{'n_envs': 2, 'n_steps': 4\}, this one is 2 envs x 5 steps"):
        Saved.load(path, env2, student2, _RawTeacher(), n_steps=5, **kwargs2)


# ---------------------------------------------------------------- the mix twin
def _run_mix(num_envs, act_dim, offset, beta, calls=R.MIX_CALLS, ids_from=0, **kw):
    low, high = R.mix_bounds(act_dim)
    twin = R.MixTwin(num_envs, low, high, seed=R.MIX_SEED, env_id_offset=offset + ids_from, beta=beta, **kw)
    out = []
    for c in range(calls):
        label, student = R.mix_inputs(num_envs, act_dim, c, offset + ids_from)
        out.append(twin.step(label, student))
    return out


def test_the_mix_twin_does_not_depend_on_batch_sharding_or_where_the_ids_start():
    whole = _run_mix(64, 3, R.MIX_OFFSET, 0.5)
    halves = [_run_mix(32, 3, R.MIX_OFFSET, 0.5, ids_from=k) for k in (0, 32)]
    for c in range(R.MIX_CALLS):
        for which in (0, 1):
            assert np.array_equal(np.concatenate([halves[0][c][which], halves[1][c][which]]), whole[c][which])
    # a larger batch: the first 64 envs are the same
    more = _run_mix(257, 3, R.MIX_OFFSET, 0.5)
    assert all(np.array_equal(more[c][1][:64], whole[c][1]) for c in range(R.MIX_CALLS))
    # the ids cross 2^32 inside the batch: env 40 has id 2^32 exactly, and draws as (lo 0, hi 1)
    alone = _run_mix(1, 3, 1 << 32, 0.5)
    assert all(alone[c][1][0] == whole[c][1][40] for c in range(R.MIX_CALLS))
    low_word_only = _run_mix(1, 3, 0, 0.5)
    assert any(low_word_only[c][1][0] != alone[c][1][0] for c in range(R.MIX_CALLS)), "the high id word is part of the counter"
    # beta's ends are exact
    assert all(d.all() for _, d in _run_mix(65, 3, R.MIX_OFFSET, 1.0)) and not any(d.any() for _, d in _run_mix(65, 3, R.MIX_OFFSET, 0.0))


def test_at_beta_one_half_every_call_of_the_gpu_test_has_both_drivers():
    """A condition on the GPU test's inputs: at every size >= 63 each of the 40 calls has an env the teacher drives and one
    it does not, so a kernel that ignored the draw, the threshold or the counter fails there."""
    for num_envs in (n for n in R.MIX_SIZES if n >= 63):
        previous = None
        for c, (_, drove) in enumerate(_run_mix(num_envs, 1, R.MIX_OFFSET, 0.5)):
            assert 0 < int(drove.sum()) < num_envs, (num_envs, c)
            assert previous is None or not np.array_equal(drove, previous), "the counter moves the draw"
            previous = drove


def test_the_mix_inputs_tell_an_inverted_drove():
    for num_envs, act_dim in R.mix_cases():
        good, bad = _run_mix(num_envs, act_dim, R.MIX_OFFSET, 0.5, calls=8), _run_mix(num_envs, act_dim, R.MIX_OFFSET, 0.5, calls=8, mutation="drove_inverted")
        for (applied, drove), (applied_bad, drove_bad) in zip(good, bad):
            assert not np.array_equal(drove, drove_bad) and not np.array_equal(applied, applied_bad), "bit-equality is the bound: any change shows"
    # and the inputs reach past the bounds on both sides, so a missing clamp shows
    label, student = R.mix_inputs(64, 3, 0, R.MIX_OFFSET)
    low, high = R.mix_bounds(3)
    for rows in (label, student):
        assert (rows < low).any() and (rows > high).any()


# ---------------------------------------------------------------- the gradient inputs tell the likely mistakes
@pytest.mark.parametrize("index,row", ROWS)
def test_the_gradient_inputs_tell_one_line_mistakes_from_the_feature(index, row):
    """On the row's inputs each mistake moves a checked output of the twin by at least 100 of the bounds the GPU test
    applies: the relative Frobenius distance of an actor tensor's gradient (bound 1e-5), the loss (rtol 1e-4, atol 1e-6),
    or a critic word's moment (held to exactly 0)."""
    shape, sources, obs, labels = R.gradient_case(index, row)
    total, A = len(obs), row.act_dim
    perm = np.random.default_rng(3).permutation(total)
    sl = R.actor_slice(shape)

    def run(mutation=None):
        x, y = R.gather(obs, labels, perm, 0, total, mutation)
        return R.minibatch(shape, sources, x, y, mutation=mutation)

    loss, grads, _ = run()
    assert np.median(np.abs(R.mean_of(shape, sources, obs) - labels)) >= 0.1, "the labels are far from the student's mean"
    assert (np.abs(R.mean_of(shape, sources, obs)) > R.ACTION_BOUND).any(), "the clamp would bite"

    def moved(mutation):
        m_loss, m_grads, _ = run(mutation)
        rel = max(np.linalg.norm(a - b) / np.linalg.norm(b) for a, b in zip(m_grads[sl], grads[sl]))
        return rel / GRAD_BOUND, abs(m_loss - loss) / (1e-4 * abs(loss) + 1e-6), m_grads

    if A > 1:
        assert moved("no_one_over_a")[0] >= 100
    assert max(moved("clamped_mean")[:2]) >= 100
    if total > 1:
        assert max(moved("label_unpermuted")[:2]) >= 100
    critic = moved("critic_gradient")[2][sl.stop:]
    assert all(np.any(g) for g in critic), "every critic tensor would show a moment where exactly 0 is demanded"


def test_a_row_with_several_actions_exists_for_the_missing_one_over_a():
    assert sum(r.act_dim > 1 for r in S.MATRIX) >= 5 and any(r.act_dim == 1 for r in S.MATRIX)
