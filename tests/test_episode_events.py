"""The episode events without a GPU: the fp64 twin (tests/episode_events_reference.py) pinned to the oracle at episode 0
and for every push, its invariance to the batch and the sharding, the properties of the push schedule, that the inputs
of tests/test_episode_events_gpu.py tell three one-line bugs from the stage, the refusals of Python and of the library,
and where `AgentStep` calls the stage."""

import ctypes as C

import numpy as np
import pytest
import torch

import upkie_amd.envs as envs
from tests import episode_events_reference as R
from tests.agent_step_doubles import D, N, T, Calls, Env, Pipeline, Policy, Reward
from tests.fake_sim import oracle_sim_factory
from tests.helpers import randomized_config
from upkie_amd import abi, lib
from upkie_amd.events import EpisodeEvents, events_params
from upkie_amd.exceptions import UpkieRuntimeError
from upkie_amd.model.default_model import default_model
from upkie_amd.model.model import Model


@pytest.fixture(scope="module")
def urdf_model():
    return Model().struct  # 13 links behind 7 bodies


def _oracle(model, num_envs, offset, seed):
    from oracle import oracle as O

    cfg = randomized_config(num_envs, seed=seed)
    cfg.env_id_offset = offset
    return O.Oracle(model, cfg)


# ---------------------------------------------------------------- the twin is the oracle where the oracle speaks
def test_the_numpy_philox_is_the_oracles():
    from oracle import oracle as O

    rng = np.random.default_rng(0)
    words = rng.integers(0, 2 ** 32, size=(6, 50), dtype=np.uint64).astype(np.uint32)
    for k in (0, 0xDEADBEEF12345678):
        got = R.philox4x32_10(words[0], words[1], words[2], words[3], k & 0xFFFFFFFF, k >> 32)
        for i in range(50):
            want = O.philox([int(words[j][i]) for j in range(4)], [k & 0xFFFFFFFF, k >> 32])
            assert [int(g[i]) for g in got] == want


@pytest.mark.parametrize("offset", (0, 1000, 2 ** 32 - 16))
@pytest.mark.parametrize("which", ("urdf", "default"))
def test_episode_zero_is_the_oracles_randomize_inertias(urdf_model, which, offset):
    model = urdf_model if which == "urdf" else default_model()
    oracle = _oracle(model, 64, offset, seed=31)
    want = oracle.sample_body_inertials(0.3)
    twin = R.Twin(model, 64, seed=31, env_id_offset=offset, inertia_variation=0.3)
    np.testing.assert_allclose(twin.body_inertials, want, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(twin.link_scale, oracle.link_scale, rtol=1e-12, atol=0.0)
    assert np.std(twin.link_scale[1:7]) > 0.1


@pytest.mark.parametrize("offset", (0, 1000, 2 ** 32 - 16))
def test_the_kth_push_is_the_oracles(urdf_model, offset):
    oracle = _oracle(urdf_model, 64, offset, seed=5)
    twin = R.Twin(urdf_model, 64, seed=5, env_id_offset=offset, push_prob=1.0, push_norm=(0.0, 20.0))
    every = np.arange(64)
    for k in (0, 1, 7, 12345):
        np.testing.assert_allclose(twin.push(every, np.uint32(k)), oracle.sample_pushes(k, 20.0), rtol=1e-12, atol=0.0)
    # ... and the stage hands them out in order: with push_prob = 1 and one-step pushes, call c starts push c of every env
    for c in range(3):
        happened = twin.step()
        assert happened["start"].all() and np.array_equal(twin.pushes, np.full(64, c + 1, dtype=np.uint32))
        np.testing.assert_allclose(twin.force, oracle.sample_pushes(c, 20.0), rtol=1e-12, atol=0.0)


# ---------------------------------------------------------------- batch and sharding invariance
def _trace(twin, terminated, truncated):
    out = []
    for t in range(len(terminated)):
        twin.step(terminated[t], truncated[t])
        out.append(twin.snapshot())
    return out


def test_a_batch_of_64_is_two_shards_of_32_and_an_env_ignores_the_others(urdf_model):
    term, trunc = R.gpu_flags(64, 0)
    kw = dict(seed=R.GPU_SEED, **R.GPU_SETTINGS)
    whole = _trace(R.Twin(urdf_model, 64, env_id_offset=0, **kw), term, trunc)
    for lo in (0, 32):
        shard = _trace(R.Twin(urdf_model, 32, env_id_offset=lo, **kw), term[:, lo:lo + 32], trunc[:, lo:lo + 32])
        for a, b in zip(whole, shard):
            for name in a:
                assert np.array_equal(a[name][..., lo:lo + 32], b[name]), name
    # other envs' flags: env 5 sees the same whatever envs 0-4 and 6-63 do
    other_term, other_trunc = R.gpu_flags(64, 77)
    other_term[:, 5], other_trunc[:, 5] = term[:, 5], trunc[:, 5]
    assert not np.array_equal(other_term, term)
    other = _trace(R.Twin(urdf_model, 64, env_id_offset=0, **kw), other_term, other_trunc)
    assert any(not np.array_equal(a["remaining"], b["remaining"]) for a, b in zip(whole, other))
    for a, b in zip(whole, other):
        for name in a:
            assert np.array_equal(a[name][..., 5], b[name][..., 5]), name


# ---------------------------------------------------------------- the schedule
def test_one_step_pushes_are_independent_draws_at_the_rate_asked_for(urdf_model):
    twin = R.Twin(urdf_model, 64, seed=3, push_prob=0.25, push_steps=(1, 1))
    starts = np.array([twin.step()["start"] for _ in range(2000)])
    n = starts.size
    assert abs(starts.mean() - 0.25) < 4.0 * np.sqrt(0.25 * 0.75 / n), starts.mean()
    # a start does not depend on the step before: the rate after a start is the rate after none
    after_start, after_none = starts[1:][starts[:-1]], starts[1:][~starts[:-1]]
    se = np.sqrt(0.25 * 0.75 * (1.0 / after_start.size + 1.0 / after_none.size))
    assert abs(after_start.mean() - after_none.mean()) < 4.0 * se
    assert np.array_equal(twin.pushes, starts.sum(axis=0).astype(np.uint32)) and np.all(twin.calls == 2000)


def test_a_three_step_push_is_held_three_steps_unless_the_episode_ends(urdf_model):
    rng = np.random.default_rng(4)
    twin = R.Twin(urdf_model, 64, seed=3, push_prob=0.2, push_steps=(3, 3), push_norm=(5.0, 20.0))
    age = np.full(64, -1)  # steps the current force has acted; -1: none
    held_full, cuts = 0, 0
    for _ in range(400):
        before = twin.force.copy()
        done = rng.random(64) < 0.03
        happened = twin.step(done, None)
        ended = (age >= 0) & ~happened["hold"]  # the force that acted so far is over (replaced by a new push or by zero)
        assert np.all((age[ended] == 2) | done[ended]), "a force ends after exactly three steps, or with its episode"
        assert np.all(age[happened["hold"]] < 2) and np.array_equal(before[:, happened["hold"]], twin.force[:, happened["hold"]])
        assert not np.any(happened["hold"] & done), "a push does not outlive its episode"
        held_full += int(np.sum(ended & (age == 2) & ~done))
        cuts += int(np.sum(happened["cut"]))
        age = np.where(happened["start"], 0, np.where(happened["hold"], age + 1, -1))
        assert np.all(np.hypot(twin.force[0], twin.force[1])[happened["start"]] >= 5.0) and np.all(twin.force[:, happened["zero"]] == 0.0)
    assert held_full > 100 and cuts > 10


def test_with_probability_one_every_free_step_starts_a_push(urdf_model):
    twin = R.Twin(urdf_model, 16, seed=3, push_prob=1.0, push_steps=(1, 4))
    for _ in range(200):
        happened = twin.step()
        assert not happened["zero"].any() and np.array_equal(happened["start"], ~happened["hold"])
    never = R.Twin(urdf_model, 16, seed=3, push_prob=0.0, inertia_variation=0.1)
    assert not any(never.step()["start"].any() for _ in range(200)) and np.all(never.force == 0.0)


# ---------------------------------------------------------------- the GPU test's inputs discriminate
@pytest.mark.parametrize("num_envs,offset", R.GPU_SIZES)
def test_the_gpu_tests_inputs_tell_three_bugs_from_the_stage(urdf_model, num_envs, offset):
    term, trunc = R.gpu_flags(num_envs, offset)
    kw = dict(seed=R.GPU_SEED, env_id_offset=offset, **R.GPU_SETTINGS)
    twin = R.Twin(urdf_model, num_envs, **kw)
    seen = {name: 0 for name in ("start", "hold", "zero", "cut")}
    redraws = np.zeros(num_envs, dtype=int)
    trace = []
    for t in range(R.GPU_CALLS):
        happened = twin.step(term[t], trunc[t])
        for name in seen:
            seen[name] += int(happened[name].sum())
        redraws += happened["redrawn"]
        trace.append(twin.snapshot())
    if num_envs >= 63:  # (one env alone cannot be asked to meet every case in 40 calls: the five larger batches each do)
        assert all(seen.values()), seen
        assert redraws.max() >= 2
        for mutation in R.MUTATIONS:
            mutant = _trace(R.Twin(urdf_model, num_envs, mutation=mutation, **kw), term, trunc)
            differs = any(not np.array_equal(a[name], b[name]) for a, b in zip(trace, mutant) for name in a)
            assert differs, mutation


# ---------------------------------------------------------------- refusals
BAD_SETTINGS = [
    (dict(push_prob=-0.1), "push_prob"), (dict(push_prob=1.5), "push_prob"), (dict(push_prob=float("nan")), "push_prob"),
    (dict(push_norm=(-1.0, 5.0)), "push_norm"), (dict(push_norm=(6.0, 5.0)), "push_norm"), (dict(push_norm=(0.0, float("inf"))), "push_norm"),
    (dict(push_norm=(float("nan"), 5.0)), "push_norm"),
    (dict(push_steps=(0, 3)), "push_steps"), (dict(push_steps=(4, 3)), "push_steps"), (dict(push_steps=(1, 65536)), "push_steps"),
    (dict(inertia_variation=-0.1), "inertia_variation"), (dict(inertia_variation=1.0), "inertia_variation"),
    (dict(inertia_variation=float("nan")), "inertia_variation"),
    (dict(push_prob=0.0, inertia_variation=0.0), "nothing to do"),
]


class _NoDeviceEnv:
    """An env whose handle must not be touched by a refused construction."""

    num_envs, device = 4, torch.device("cuda:0")

    def __init__(self):
        self.model = Model()

    @property
    def sim(self):
        raise AssertionError("a refused construction touched the simulation handle")


def test_python_refuses_every_listed_limit_before_any_device_use():
    env = _NoDeviceEnv()
    ok = dict(push_prob=0.25)
    for change, match in BAD_SETTINGS:
        with pytest.raises(ValueError, match=match):
            EpisodeEvents(env, **dict(ok, **change))
    with pytest.raises(ValueError, match="push_steps"):
        EpisodeEvents(env, push_prob=0.25, push_steps=(1.5, 3))
    with pytest.raises(ValueError, match="no link named 'elbow'"):
        EpisodeEvents(env, push_prob=0.25, push_link="elbow")
    p = events_params(0.25, (5.0, 20.0), (1, 3), 0.3)
    assert (p.push_prob, p.push_norm_min, p.push_norm_max, p.push_steps_min, p.push_steps_max, p.inertia_variation) == (0.25, 5.0, 20.0, 1, 3, 0.3)
    # a CPU env (the oracle behind the handle's interface) is refused: there is no CPU fallback
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=3, sim_factory=oracle_sim_factory) as cpu_env:
        assert cpu_env.device.type == "cpu"
        with pytest.raises(UpkieRuntimeError, match="no CPU fallback"):
            EpisodeEvents(cpu_env, push_prob=0.25)


@pytest.fixture(scope="module")
def library():
    lib.build()
    return lib.load()


def test_library_refuses_every_listed_limit_without_a_gpu(library):
    for name in ("upkie_sim_episode_events_step", "upkie_sim_episode_events_reset"):
        assert name in lib.EXPORTED_SYMBOLS and getattr(library, name) is not None
    assert abi.STRUCT_IDS[11] is abi.UpkieEpisodeEvents and library.upkie_hip_struct_bytes(11) == C.sizeof(abi.UpkieEpisodeEvents)
    err = lambda: library.upkie_sim_last_error(None)  # noqa: E731
    buf = (C.c_uint32 * 64)()
    fake_handle = None  # (every refusal below comes before the handle is read)

    def params(**change):
        p = abi.UpkieEpisodeEvents()
        p.push_prob, p.push_norm_min, p.push_norm_max, p.push_steps_min, p.push_steps_max, p.inertia_variation = 0.25, 0.0, 20.0, 1, 1, 0.0
        for name, value in change.items():
            if name == "push_norm":
                p.push_norm_min, p.push_norm_max = value
            elif name == "push_steps":
                p.push_steps_min, p.push_steps_max = value
            else:
                setattr(p, name, value)
        return p

    def step(p):
        return library.upkie_sim_episode_events_step(fake_handle, C.byref(p), None, None, buf, buf, buf, buf, buf, None, None, None)

    def reset(p):
        return library.upkie_sim_episode_events_reset(fake_handle, C.byref(p), None, buf, buf, buf, buf, buf, None, None, None)

    for call in (step, reset):
        for change, word in BAD_SETTINGS:
            assert call(params(**change)) == abi.ERR_INVALID_ARGUMENT, (call.__name__, change)
            assert word.encode() in err(), (call.__name__, change, err())
        # good settings and no handle: refused as a null argument, and never launched
        assert call(params()) == abi.ERR_INVALID_ARGUMENT and b"null argument" in err()
    assert library.upkie_sim_episode_events_step(None, None, None, None, buf, buf, buf, buf, buf, None, None, None) == abi.ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- where AgentStep calls the stage
class _Events:
    def __init__(self, calls, num_envs=N):
        self.calls, self.num_envs = calls, num_envs

    def reset(self):
        self.calls.add("events.reset")

    def step(self, terminated, truncated):
        self.calls.add("events.step", terminated=terminated, truncated=truncated)


@pytest.mark.parametrize("pipeline", (False, True))
def test_agent_step_steps_the_events_after_the_reward_and_before_observe(pipeline):
    from upkie_amd.agent_step import AgentStep
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    calls = Calls()
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=N, frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=4,
                   sim_factory=oracle_sim_factory) as inner:
        pipe = Pipeline(calls) if pipeline else None
        policy = Policy(pipe.stacked_dim if pipeline else D, calls)
        agent = AgentStep(Env(inner, calls), policy, pipe, Reward(D, calls), events=_Events(calls))
        agent.reset(seed=0)
        assert calls.names == ["env.reset"] + (["pipeline.reset"] if pipeline else []) + ["events.reset"]
        del calls.names[:]
        action = torch.zeros(N, 1)
        for _ in range(T):
            agent.apply(action)
            agent.observe()
        assert calls.names == ((["shape_action"] if pipeline else []) + ["env.step", "reward.step", "events.step"] + (["observe"] if pipeline else [])) * T
        for k in range(T):
            out = calls.args["env.step"][k]["out"]
            assert calls.args["events.step"][k]["terminated"] is out[2] and calls.args["events.step"][k]["truncated"] is out[3]
        with pytest.raises(ValueError, match="the events serve 5 envs"):
            AgentStep(Env(inner, calls), policy, pipe, events=_Events(calls, num_envs=5))
        # without events nothing is called that was not before
        del calls.names[:]
        plain = AgentStep(Env(inner, calls), policy, pipe, Reward(D, calls))
        plain.reset()
        plain.apply(action)
        assert not any(name.startswith("events") for name in calls.names)


def test_ppo_and_the_evaluator_pass_their_events_to_the_agent_step(monkeypatch):
    import upkie_amd.evaluation as evaluation
    from tests.agent_step_doubles import Tally
    from upkie_amd.evaluation import EvalCallback, PolicyEvaluator
    from upkie_amd.ppo import Ppo

    calls = Calls()
    monkeypatch.setattr(evaluation, "EpisodeTally", lambda num_envs, capacity, device: Tally(calls, num_envs, capacity))
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=N, autoreset_mode="same_step", max_episode_steps=4, sim_factory=oracle_sim_factory) as inner:
        events = _Events(calls)
        model = Ppo(inner, Policy(D, calls), events=events)
        assert model.events is events and model._agent.events is events and Ppo._FILE_NAMES["events"] == ("events.", {})
        assert Ppo(inner, Policy(D, calls)).events is None
        runner = PolicyEvaluator(Policy(D, calls), inner, 3, graph=False, events=events)
        assert runner.events is events and runner._agent.events is events
        assert EvalCallback(inner, events=events).events is events
