"""The task targets without a GPU: the refusals of Python and of the library, the header against abi.py, the properties of
the fp64 twin (tests/task_targets_reference.py) over 20000 draws, its invariance to the batch and the sharding, the
curriculum twin, that the inputs of tests/test_task_targets_gpu.py tell five one-line bugs from the stage, and where
`AgentStep`, `Ppo` and the evaluator call the stage."""

import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import upkie_amd.envs as envs
from tests import task_targets_reference as R
from tests.agent_step_doubles import A, D, N, T, Calls, Env, Pipeline, Policy, Reward
from tests.fake_sim import oracle_sim_factory
from upkie_amd import abi, lib
from upkie_amd.exceptions import UpkieRuntimeError
from upkie_amd.targets import TargetCurriculum, TaskTargets, targets_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------- refusals
# (what changes in otherwise good settings, the word the message carries)
BAD_SETTINGS = [
    (dict(num_targets=0), "targets"), (dict(num_targets=9), "targets"), (dict(obs_dim=0), "obs_dim"), (dict(obs_dim=255, num_targets=2), "obs_dim"),
    (dict(obs_dim=249, num_targets=8), "obs_dim"),
    (dict(resample_steps=(0, 3)), "resample_steps"), (dict(resample_steps=(4, 3)), "resample_steps"), (dict(resample_steps=(1, 65536)), "resample_steps"),
    (dict(stand_prob=-0.1), "stand_prob"), (dict(stand_prob=1.5), "stand_prob"), (dict(stand_prob=float("nan")), "stand_prob"),
    (dict(deadband=[-0.1, 0.0]), "deadband"), (dict(deadband=[float("inf"), 0.0]), "deadband"), (dict(deadband=[float("nan"), 0.0]), "deadband"),
]


class _NoDeviceEnv:
    """An env whose handle must not be touched by a refused construction."""

    num_envs, device = 4, torch.device("cuda:0")
    single_observation_space = type("Space", (), {"shape": (6,)})()

    @property
    def sim(self):
        raise AssertionError("a refused construction touched the simulation handle")


def test_python_refuses_every_listed_limit_before_any_device_use():
    env = _NoDeviceEnv()
    ok = dict(obs_dim=6, num_targets=2, resample_steps=(1, 3), stand_prob=0.1, deadband=[0.0, 0.0])
    for change, match in BAD_SETTINGS:
        with pytest.raises(ValueError, match=match):
            targets_params(**dict(ok, **change))
    p = targets_params(6, 2, (2, 5), 0.25, [0.05, 0.0])
    assert (p.obs_dim, p.num_targets, p.resample_steps_min, p.resample_steps_max, p.stand_prob, p.deadband[0], p.deadband[1]) == (6, 2, 2, 5, 0.25, 0.05, 0.0)
    assert targets_params(248, 8).obs_dim == 248  # (the cap itself is served)
    names9 = tuple(f"t{g}" for g in range(9))
    for kw, match in ((dict(names=()), "targets"), (dict(names=names9, ranges=[(-1, 1)] * 9), "targets"), (dict(obs_dim=255), "obs_dim"),
                      (dict(ranges=[(1.0, -1.0), (-1, 1)]), "low <= high"), (dict(ranges=[(-1, 1)]), "one pair"),
                      (dict(ranges=[(-1, float("inf")), (-1, 1)]), "finite"), (dict(ranges=[(float("nan"), 1), (-1, 1)]), "finite"),
                      (dict(resample_steps=(0, 3)), "resample_steps"), (dict(resample_steps=(1.5, 3)), "resample_steps"),
                      (dict(stand_prob=1.5), "stand_prob"), (dict(deadband=[0.1]), "deadband"), (dict(names=("a", "a")), "differ")):
        with pytest.raises(ValueError, match=match):
            TaskTargets(env, **dict(dict(resample_steps=(1, 3)), **kw))
    for kw, match in ((dict(step=[0.1, -0.1]), "step"), (dict(step=[0.1, float("nan")]), "step"), (dict(limit=[(1, -1), (-1, 1)]), "low <= high"),
                      (dict(limit=[(-1, 1)]), "one pair"), (dict(limit=[(-1, float("inf")), (-1, 1)]), "finite"), (dict(threshold=float("nan")), "threshold")):
        with pytest.raises(ValueError, match=match):
            TargetCurriculum(**dict(dict(term="track", threshold=1.0, step=[0.1, 0.1], limit=[(-2, 2), (-2, 2)]), **kw))
    curriculum = TargetCurriculum("track", 1.0, [0.1, 0.1], [(-0.5, 0.5), (-2, 2)])
    with pytest.raises(ValueError, match="within the curriculum's limit"):
        TaskTargets(env, resample_steps=(1, 3), curriculum=curriculum)
    with pytest.raises(ValueError, match="the curriculum has 1 steps"):
        TaskTargets(env, resample_steps=(1, 3), curriculum=TargetCurriculum("track", 1.0, [0.1], [(-2, 2)]))
    # a CPU env (the oracle behind the handle's interface) is refused: there is no CPU fallback
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=3, sim_factory=oracle_sim_factory) as cpu_env:
        assert cpu_env.device.type == "cpu"
        with pytest.raises(UpkieRuntimeError, match="no CPU fallback"):
            TaskTargets(cpu_env, resample_steps=(1, 3))


@pytest.fixture(scope="module")
def library():
    lib.build()
    return lib.load()


def test_library_refuses_every_listed_limit_without_a_gpu(library):
    for name in ("upkie_sim_task_targets_step", "upkie_sim_task_targets_reset", "upkie_sim_task_targets_curriculum",
                 "upkie_sim_task_targets_workspace_bytes"):
        assert name in lib.EXPORTED_SYMBOLS and getattr(library, name) is not None
    assert abi.STRUCT_IDS[12] is abi.UpkieTaskTargets and library.upkie_hip_struct_bytes(12) == C.sizeof(abi.UpkieTaskTargets)
    err = lambda: library.upkie_sim_last_error(None)  # noqa: E731
    buf = (C.c_uint32 * 64)()

    def params(**change):
        p = abi.UpkieTaskTargets()
        p.obs_dim, p.num_targets, p.resample_steps_min, p.resample_steps_max, p.stand_prob = 6, 2, 1, 3, 0.1
        for name, value in change.items():
            if name == "resample_steps":
                p.resample_steps_min, p.resample_steps_max = value
            elif name == "deadband":
                for g, v in enumerate(value):
                    p.deadband[g] = v
            else:
                setattr(p, name, value)
        return p

    def step(p):  # (a NULL handle: every refusal of a setting comes before the handle is read)
        return library.upkie_sim_task_targets_step(None, C.byref(p), buf, None, None, None, buf, buf, buf, buf, buf, buf, None)

    def reset(p):
        return library.upkie_sim_task_targets_reset(None, C.byref(p), buf, None, buf, buf, buf, buf, buf, None)

    for call in (step, reset):
        for change, word in BAD_SETTINGS:
            assert call(params(**change)) == abi.ERR_INVALID_ARGUMENT, (call.__name__, change)
            assert word.encode() in err(), (call.__name__, change, err())
        # good settings and no handle: refused as a null argument, and never launched
        assert call(params()) == abi.ERR_INVALID_ARGUMENT and b"null argument" in err()
    assert library.upkie_sim_task_targets_step(None, None, buf, None, None, None, buf, buf, buf, buf, buf, buf, None) == abi.ERR_INVALID_ARGUMENT
    assert b"null argument" in err()

    def curriculum(G=2, threshold=1.0, step=(0.1, 0.1), limit=(-2.0, 2.0, -2.0, 2.0)):
        return library.upkie_sim_task_targets_curriculum(None, G, threshold, (C.c_float * 8)(*step), (C.c_float * 16)(*limit), buf, buf, buf, buf, buf, None)

    for kw, word in ((dict(G=0), b"num_targets"), (dict(G=9), b"num_targets"), (dict(threshold=float("nan")), b"threshold"),
                     (dict(step=(0.1, -0.1)), b"step"), (dict(step=(float("inf"), 0.1)), b"step"), (dict(limit=(2.0, -2.0, -2.0, 2.0)), b"limit"),
                     (dict(limit=(-2.0, 2.0, -2.0, float("nan"))), b"limit"), (dict(), b"null argument")):
        assert curriculum(**kw) == abi.ERR_INVALID_ARGUMENT and word in err(), (kw, err())
    assert library.upkie_sim_task_targets_workspace_bytes(0) == abi.ERR_INVALID_ARGUMENT
    # the ticket, then a (sum, count) pair per block of 2048 envs
    assert [library.upkie_sim_task_targets_workspace_bytes(n) for n in (1, 2048, 2049, 4097)] == [24, 24, 40, 56]


def test_the_header_and_abi_py_agree():
    probe = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "upkie_hip.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(UpkieTaskTargets), offsetof(UpkieTaskTargets, stand_prob), offsetof(UpkieTaskTargets, deadband),
             offsetof(UpkieTaskTargets, obs_dim), offsetof(UpkieTaskTargets, num_targets), offsetof(UpkieTaskTargets, resample_steps_min),
             offsetof(UpkieTaskTargets, resample_steps_max), UPKIE_TASK_TARGETS_MAX, UPKIE_STRUCT_TASK_TARGETS);
      return 0;
    }
    """
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write(probe)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    t = abi.UpkieTaskTargets
    assert got == [C.sizeof(t), t.stand_prob.offset, t.deadband.offset, t.obs_dim.offset, t.num_targets.offset, t.resample_steps_min.offset,
                   t.resample_steps_max.offset, abi.TASK_TARGETS_MAX, 12]
    with open(os.path.join(ROOT, "upkie_amd", "csrc", "random.hpp")) as f:
        assert int(re.search(r"STREAM_TARGETS = (\d+)", f.read()).group(1)) == R.STREAM_TARGETS == 7
    with open(os.path.join(ROOT, "include", "upkie_hip.h")) as f:
        assert "STREAM_TARGETS = 7" in f.read()


# ---------------------------------------------------------------- the twin's properties
def _run(twin, calls, p_done=0.05, seed=0):
    """``calls`` steps on zero observations with random end flags; per call (snapshot, what happened, target before)."""
    rng = np.random.default_rng(seed)
    obs = np.zeros((twin.N, twin.D))
    twin.reset(obs)
    out = []
    for _ in range(calls):
        before = twin.target.copy()
        happened = twin.step(obs, rng.random(twin.N) < p_done, None)
        out.append((twin.snapshot(), happened, before))
    return out


def test_draws_lie_in_their_ranges_holds_in_resample_steps_and_stands_come_at_the_rate_asked_for():
    ranges = [(-0.3, 0.7), (2.0, 2.5), (-1.0, -0.25), (0.0, 0.0), (-4.0, 4.0)]
    twin = R.Twin(100, 3, ranges, seed=5, resample_steps=(2, 6), stand_prob=0.3)
    draws = stands = 0
    hold_seen = set()
    age = np.ones(100, dtype=int)  # observations the current target has been in (the reset row is the first)
    for snap, happened, before in _run(twin, 1000):
        drawn = happened["drawn"]
        x = snap["target"][:, drawn]
        stand = np.all(x == 0.0, axis=0)
        for g, (lo, hi) in enumerate(np.asarray(ranges, dtype=np.float32).astype(np.float64)):
            assert np.all((x[g][~stand] >= lo) & (x[g][~stand] <= hi)), g
        draws, stands = draws + int(drawn.sum()), stands + int(stand.sum())
        assert np.array_equal(snap["target"][:, ~drawn], before[:, ~drawn]), "a held target does not move"
        hold = snap["remaining"][drawn]
        assert np.all((hold >= 2) & (hold <= 6))
        hold_seen |= set(hold.tolist())
        # a target is in force its hold length, unless the episode ends
        ended = age[drawn]
        assert np.all(ended <= 6) and np.all((ended >= 2) | happened["done"][drawn])
        age = np.where(drawn, 1, age + 1)
        assert np.array_equal(snap["observation"][:, 3:], snap["target"].T) and np.array_equal(snap["final_observation"][:, 3:], before.T)
    assert draws >= 20000 and hold_seen == {2, 3, 4, 5, 6}
    # (word 1's range excludes zero, so an all-zero target is a stand and nothing else)
    assert abs(stands / draws - 0.3) < 4.0 * np.sqrt(0.3 * 0.7 / draws), stands / draws


def test_a_deadband_zeroes_the_small_words_only():
    kw = dict(seed=2, resample_steps=(1, 1))
    plain = R.Twin(500, 1, [(-1.0, 1.0), (-1.0, 1.0)], **kw)
    banded = R.Twin(500, 1, [(-1.0, 1.0), (-1.0, 1.0)], deadband=[0.25, 0.0], **kw)
    a, b = _run(plain, 40), _run(banded, 40)
    small = 0
    for (sa, _, _), (sb, _, _) in zip(a, b):
        x, y = sa["target"], sb["target"]
        inside = np.abs(x[0]) < 0.25
        small += int(inside.sum())
        assert np.all(y[0][inside] == 0.0) and not np.any(np.signbit(y[0][inside])) and np.array_equal(y[0][~inside], x[0][~inside])
        assert np.array_equal(y[1], x[1])
    assert 0.2 < small / (40 * 500) < 0.3


def _trace(twin, obs0, next_obs, final_obs, terminated, truncated):
    twin.reset(obs0)
    out = [twin.snapshot()]
    for t in range(len(terminated)):
        twin.step(next_obs[t], terminated[t], truncated[t], final_obs[t])
        out.append(twin.snapshot())
    return out


def _columns(name, a, cols):
    return a[..., cols] if name == "target" else a[cols]


def test_an_envs_schedule_ignores_the_batch_the_sharding_and_the_other_envs():
    (D, G), kw = (6, 5), dict(seed=R.GPU_SEED, **R.gpu_settings(5))
    term, trunc = R.gpu_flags(64, 0)
    obs0, nxt, fin = R.gpu_observations(64, D)
    whole = _trace(R.Twin(64, D, env_id_offset=0, **kw), obs0, nxt, fin, term, trunc)
    for lo in (0, 32):
        part = slice(lo, lo + 32)
        shard = _trace(R.Twin(32, D, env_id_offset=lo, **kw), obs0[part], nxt[:, part], fin[:, part], term[:, part], trunc[:, part])
        for a, b in zip(whole, shard):
            for name in a:
                assert np.array_equal(_columns(name, a[name], part), b[name]), name
    # an id offset split: ids 2^32 - 16 ... 2^32 + 47 as one batch and as the two sides of the carry
    big = 2 ** 32 - 16
    whole = _trace(R.Twin(64, D, env_id_offset=big, **kw), obs0, nxt, fin, term, trunc)
    for lo, n in ((0, 16), (16, 48)):
        part = slice(lo, lo + n)
        shard = _trace(R.Twin(n, D, env_id_offset=big + lo, **kw), obs0[part], nxt[:, part], fin[:, part], term[:, part], trunc[:, part])
        for a, b in zip(whole, shard):
            for name in a:
                assert np.array_equal(_columns(name, a[name], part), b[name]), name
    # other envs' flags: env 5 sees the same whatever the others do
    other_term, other_trunc = R.gpu_flags(64, 77)
    other_term[:, 5], other_trunc[:, 5] = term[:, 5], trunc[:, 5]
    other = _trace(R.Twin(64, D, env_id_offset=big, **kw), obs0, nxt, fin, other_term, other_trunc)
    assert any(not np.array_equal(a["remaining"], b["remaining"]) for a, b in zip(whole, other))
    for a, b in zip(whole, other):
        for name in ("calls", "remaining", "target", "observation"):
            assert np.array_equal(_columns(name, a[name], 5), _columns(name, b[name], 5)), name


# ---------------------------------------------------------------- the curriculum twin
def test_the_curriculum_widens_only_above_the_threshold_clamps_and_ignores_envs_with_nothing_new():
    S = R.CURRICULUM_SETTINGS
    for num_envs in R.CURRICULUM_SIZES:
        score, finished = R.curriculum_inputs(num_envs)
        assert np.all(score * 1024 == np.round(score * 1024)) and np.abs(score).max() * num_envs < 2 ** 20 * 4097
        limits, seen = np.asarray(S["ranges"], dtype=np.float32), np.zeros(num_envs, dtype=np.int32)
        moved, trace = [], []
        for k in range(6):
            moved.append(R.curriculum_step(limits, seen, score[k], finished[k], S["threshold"], S["step"], S["limit"]))
            trace.append(limits.copy())
            assert np.array_equal(seen, finished[k])
        assert moved == [True, False, True, True, False, False]
        assert trace[0].tolist() == [[-0.75, 0.75]] * 2 and trace[1].tolist() == trace[0].tolist() and trace[2].tolist() == [[-1.0, 1.0]] * 2
        assert trace[3].tolist() == [[-1.0, 1.125]] * 2 and trace[5].tolist() == trace[3].tolist()  # (clamped on both sides)
        # counting every env (no `seen`) would have decided otherwise
        assert score[0].mean() < S["threshold"] or num_envs == 1


# ---------------------------------------------------------------- the GPU test's inputs discriminate
@pytest.mark.parametrize("D,G", R.GPU_WIDTHS)
@pytest.mark.parametrize("num_envs,offset", R.GPU_SIZES)
def test_the_gpu_tests_inputs_tell_five_bugs_from_the_stage(num_envs, offset, D, G):
    term, trunc = R.gpu_flags(num_envs, offset)
    obs0, nxt, fin = R.gpu_observations(num_envs, D)
    kw = dict(seed=R.GPU_SEED, env_id_offset=offset, **R.gpu_settings(G))
    trace = _trace(R.Twin(num_envs, D, **kw), obs0, nxt, fin, term, trunc)
    if num_envs < 63:  # (one env alone cannot be asked to meet every case in 40 calls: the larger batches each do)
        return
    for mutation in R.MUTATIONS:
        if mutation == "block_one_for_words_above_four" and G <= 4:
            continue  # (no word above four: the bug cannot show)
        mutant = _trace(R.Twin(num_envs, D, mutation=mutation, **kw), obs0, nxt, fin, term, trunc)
        differs = any(not np.array_equal(a[name], b[name]) for a, b in zip(trace, mutant) for name in a)
        assert differs, mutation


# ---------------------------------------------------------------- where AgentStep calls the stage
G2 = 2


class _Targets:
    def __init__(self, calls, num_envs=N, obs_dim=D):
        self.log, self.num_envs, self.obs_dim, self.num_targets, self.dim = calls, num_envs, obs_dim, G2, obs_dim + G2
        self.observation, self.final_observation = torch.zeros(num_envs, self.dim), torch.zeros(num_envs, self.dim)
        self.curriculum = None

    def reset(self, obs):
        self.log.add("targets.reset", obs=obs)
        return self.observation

    def step(self, next_obs, terminated, truncated, final_obs=None):
        self.log.add("targets.step", next_obs=next_obs, terminated=terminated, truncated=truncated, final_obs=final_obs)
        return self.observation


class _WidePipeline(Pipeline):
    def __init__(self, calls):
        super().__init__(calls)
        self.obs_dim = D + G2
        self.frame_dim, self.stacked_dim = D + G2 + A, 2 * (D + G2 + A)
        self.observation, self.final_observation = torch.zeros(N, self.stacked_dim), torch.zeros(N, self.stacked_dim)

    def reset(self, obs):
        self.log.add("pipeline.reset", obs=obs)
        return self.observation

    def observe(self, next_obs, terminated, truncated, final_obs=None):
        self.log.add("observe", next_obs=next_obs, terminated=terminated, truncated=truncated, final_obs=final_obs)
        return self.observation


@pytest.mark.parametrize("pipeline", (False, True))
def test_agent_step_steps_the_targets_after_the_env_and_before_the_reward(pipeline):
    from upkie_amd.agent_step import AgentStep
    from tests.test_episode_events import _Events

    calls = Calls()
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=N, frequency=200.0, autoreset_mode="same_step", max_episode_steps=4,
                   sim_factory=oracle_sim_factory) as inner:
        pipe = _WidePipeline(calls) if pipeline else None
        policy = Policy(pipe.stacked_dim if pipeline else D + G2, calls)
        targets = _Targets(calls)
        agent = AgentStep(Env(inner, calls), policy, pipe, Reward(D + G2, calls), events=_Events(calls), targets=targets)
        agent.reset(seed=0)
        assert calls.names == ["env.reset", "targets.reset"] + (["pipeline.reset"] if pipeline else []) + ["events.reset"]
        assert calls.args["targets.reset"][0]["obs"] is inner.observation
        if pipeline:
            assert calls.args["pipeline.reset"][0]["obs"] is targets.observation
        assert agent.raw_observation is targets.observation
        del calls.names[:]
        action = torch.zeros(N, 1)
        for _ in range(T):
            stepped = agent.apply(action)
            assert stepped[0] is targets.observation and stepped[4] is targets.final_observation and agent.raw_observation is targets.observation
            observed = agent.observe()
            if not pipeline:
                assert observed[0] is targets.observation and observed[1] is targets.final_observation
        assert calls.names == ((["shape_action"] if pipeline else []) + ["env.step", "targets.step", "reward.step", "events.step"]
                               + (["observe"] if pipeline else [])) * T
        for k in range(T):
            out, given = calls.args["env.step"][k]["out"], calls.args["targets.step"][k]
            assert given["next_obs"] is out[0] and given["terminated"] is out[2] and given["truncated"] is out[3]
            assert given["final_obs"] is out[4]["final_obs"]
            scored = calls.args["reward.step"][k]
            assert scored["next_obs"] is targets.final_observation and scored["final_obs"] is None  # the outcome under the old target, everywhere
            if pipeline:
                seen = calls.args["observe"][k]
                assert seen["next_obs"] is targets.observation and seen["final_obs"] is targets.final_observation
        # a reward_fn receives the same row
        from tests.agent_step_doubles import reward_fn

        with_fn = AgentStep(Env(inner, calls), policy, pipe, reward_fn=reward_fn(calls), targets=targets)
        with_fn.reset()
        with_fn.apply(action)
        assert calls.args["reward_fn"][0]["next_obs"] is targets.final_observation
        # the sizes: the raw width is the env's D + G
        with pytest.raises(ValueError, match="the targets serve 5 envs"):
            AgentStep(Env(inner, calls), policy, pipe, targets=_Targets(calls, num_envs=5))
        narrow = Pipeline(calls) if pipeline else None
        with pytest.raises(ValueError, match=f"reads {D} raw observation words, the env's {D} and the {G2} targets make {D + G2}"):
            AgentStep(Env(inner, calls), Policy(narrow.stacked_dim if pipeline else D, calls), narrow, targets=_Targets(calls))
        # without targets nothing is called that was not before
        del calls.names[:]
        plain = AgentStep(Env(inner, calls), Policy(Pipeline(calls).stacked_dim if pipeline else D, calls), Pipeline(calls) if pipeline else None,
                          Reward(D, calls))
        plain.reset()
        plain.apply(action)
        assert not any(name.startswith("targets") for name in calls.names)
        assert calls.args["reward.step"][-1]["final_obs"] is calls.args["env.step"][-1]["out"][4]["final_obs"]


def test_ppo_and_the_evaluator_pass_their_targets_to_the_agent_step(monkeypatch):
    import upkie_amd.evaluation as evaluation
    from tests.agent_step_doubles import Tally
    from upkie_amd.evaluation import EvalCallback, PolicyEvaluator
    from upkie_amd.ppo import Ppo

    calls = Calls()
    monkeypatch.setattr(evaluation, "EpisodeTally", lambda num_envs, capacity, device: Tally(calls, num_envs, capacity))
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=N, autoreset_mode="same_step", max_episode_steps=4, sim_factory=oracle_sim_factory) as inner:
        targets = _Targets(calls)
        model = Ppo(inner, Policy(D + G2, calls), targets=targets)
        assert model.targets is targets and model._agent.targets is targets and Ppo._FILE_NAMES["targets"] == ("targets.", {})
        plain = Ppo(inner, Policy(D, calls))
        assert plain.targets is None and plain._agent.targets is None and plain._curriculum_term is None
        runner = PolicyEvaluator(Policy(D + G2, calls), inner, 3, graph=False, targets=targets)
        assert runner.targets is targets and runner._agent.targets is targets
        assert EvalCallback(inner, targets=targets).targets is targets
        # a curriculum names a term of the reward, and is refused with a process group
        targets.curriculum = TargetCurriculum("track", 1.0, [0.1, 0.1], [(-2, 2), (-2, 2)])
        reward = Reward(D + G2, calls)
        reward.names = ("alive", "track")
        assert Ppo(inner, Policy(D + G2, calls), targets=targets, reward=reward)._curriculum_term == 1
        reward.names = ("alive",)
        with pytest.raises(ValueError, match="the curriculum reads the reward term 'track'"):
            Ppo(inner, Policy(D + G2, calls), targets=targets, reward=reward)
        with pytest.raises(ValueError, match="the curriculum reads the reward term 'track'"):
            Ppo(inner, Policy(D + G2, calls), targets=targets)
        with pytest.raises(ValueError, match="TargetCurriculum with a process_group"):
            Ppo(inner, Policy(D + G2, calls), targets=targets, reward=reward, process_group=object())
