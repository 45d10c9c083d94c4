"""The push curriculum without a GPU: Python's refusals by name, the header against `abi.py` and `lib.py`, the library's
refusals without a device, the fp64 twin (tests/push_curriculum_reference.py) -- the existing twin's bits with L = 0,
levels within 0..L, invariance to batch, shard and an id offset across 2^32 --, that the inputs of
tests/test_push_curriculum_gpu.py meet every branch and tell five one-line bugs from the stage, and `Ppo`'s call order
under a levelled events object."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import upkie_amd.envs as envs
from tests import episode_events_reference as R
from tests import push_curriculum_reference as P
from tests.agent_step_doubles import D, N, T, Calls, Env
from tests.fake_sim import oracle_sim_factory
from tests.test_ppo_rollout_step import STEP_CALLS, _model
from upkie_amd import abi, lib
from upkie_amd.events import EpisodeEvents, PushLevels, events_params, settings_values, settings_words
from upkie_amd.exceptions import UpkieRuntimeError
from upkie_amd.model.model import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def urdf_model():
    return Model().struct


def _trace(twin, terminated, truncated, watch=None):
    out = []
    for t in range(len(terminated)):
        happened = twin.step(terminated[t], truncated[t])
        if watch is not None:
            watch(happened)
        out.append(twin.snapshot())
    return out


def _twin(model, num_envs, offset, **kw):
    return P.LevelTwin(model, num_envs, seed=P.GPU_SEED, env_id_offset=offset, **dict(dict(P.GPU_LEVELS, **P.GPU_SETTINGS), **kw))


# ---------------------------------------------------------------- Python's refusals
BAD_LEVELS = [
    (dict(levels=-1), "levels must be in 0-255"), (dict(levels=256), "levels must be in 0-255"), (dict(levels=2.5), "levels must be a whole number"),
    (dict(levels="3"), "levels must be a whole number"), (dict(levels=True), "levels must be a whole number"),
    (dict(levels=float("nan")), "levels must be a whole number"),
    (dict(levels=3, start=4), "start must be in 0-levels"), (dict(levels=3, start=-1), "start must be in 0-levels"),
    (dict(levels=3, up=4), "up must be in 0-levels"), (dict(levels=3, down=4), "down must be in 0-levels"), (dict(levels=3, down=-1), "down must be in 0-levels"),
    (dict(levels=0), "up must be in 0-levels"),  # (the defaults move one level: say up=0, down=0 for a single level)
    (dict(levels=3, min_pushes=-1), "min_pushes must be in"), (dict(levels=3, min_pushes=2 ** 31), "min_pushes must be in"),
    (dict(levels=3, min_pushes=0.5), "min_pushes must be a whole number"),
]


class _NoDeviceEnv:
    """An env whose handle must not be touched by a refused construction."""

    num_envs, device = 4, torch.device("cuda:0")

    def __init__(self):
        self.model = Model()

    @property
    def sim(self):
        raise AssertionError("a refused construction touched the simulation handle")


def test_python_refuses_every_listed_limit_by_name():
    for settings, match in BAD_LEVELS:
        with pytest.raises(ValueError, match=match):
            PushLevels(**settings)
    ok = PushLevels(3, start=3, up=0, down=0)
    assert (ok.levels, ok.start, ok.up, ok.down, ok.min_pushes) == (3, 3, 0, 0, 1) and "levels=3" in repr(ok)
    assert (PushLevels(255, 255, 255, 255, 0).levels, PushLevels(0, up=0, down=0).levels) == (255, 0)
    env = _NoDeviceEnv()
    with pytest.raises(ValueError, match="curriculum must be a PushLevels"):
        EpisodeEvents(env, push_prob=0.25, curriculum=3)
    for live in (dict(live=True), dict(curriculum=ok)):  # (the settings' own limits hold with a block as without)
        with pytest.raises(ValueError, match="push_norm"):
            EpisodeEvents(env, push_prob=0.25, push_norm=(6.0, 5.0), **live)
        with pytest.raises(ValueError, match="nothing to do"):
            EpisodeEvents(env, **live)
    # an object built without a block refuses the three calls that need one, by name
    plain = object.__new__(EpisodeEvents)
    plain._levels = None
    for name, args in (("set_push", dict(prob=0.5)), ("set_levels", dict(levels=1)), ("level_counts", {})):
        with pytest.raises(UpkieRuntimeError, match=f"{name} needs the push settings in a device block: build the EpisodeEvents with live=True"):
            getattr(plain, name)(**args)
    plain.curriculum, plain.live = None, False
    assert plain.log() == {}, "a plain stage adds nothing to a training record"
    # a CPU env is refused as before: there is no CPU fallback
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=3, sim_factory=oracle_sim_factory) as cpu_env:
        with pytest.raises(UpkieRuntimeError, match="no CPU fallback"):
            EpisodeEvents(cpu_env, push_prob=0.25, curriculum=ok)


def test_the_block_holds_the_checked_settings_word_for_word():
    p = events_params(0.25, (P.NORM_MIN, P.NORM_MAX), (2, 5), 0.0)
    words = settings_words(p, PushLevels(3, start=1, up=1, down=2, min_pushes=4))
    assert words.dtype == torch.int32 and tuple(words.shape) == (abi.EVENTS_SETTINGS_WORDS,) == (len(abi.EVENTS_SETTINGS),)
    raw = words.numpy().view(np.uint32)
    assert [int(raw[i]) for i in (0, 3, 4, 5, 6, 7, 8)] == [2 ** 22, 2, 4, 3, 1, 2, 4]
    assert raw[1:3].view(np.float32).tolist() == [np.float32(P.NORM_MIN), np.float32(P.NORM_MAX)]
    back = settings_values(words)
    assert (back["push_prob"], back["norm_min"], back["norm_max"], back["push_steps"]) == (0.25, P.NORM_MIN, P.NORM_MAX, (2, 5))
    assert (back["levels"], back["up"], back["down"], back["min_pushes"]) == (3, 1, 2, 4)
    # every threshold survives the way there and back: llround(threshold / 2^24 * 2^24)
    for prob in (1.0, 1e-7, 0.3, 2.0 ** -24):
        w = settings_words(events_params(prob), PushLevels(0, up=0, down=0))
        again = settings_words(events_params(settings_values(w)["push_prob"]), PushLevels(0, up=0, down=0))
        assert torch.equal(w, again)


# ---------------------------------------------------------------- the header, abi.py and lib.py
def test_the_header_is_what_abi_and_lib_mirror():
    with open(os.path.join(ROOT, "include", "upkie_hip.h")) as f:
        header = f.read()
    defines = dict(re.findall(r"#define (UPKIE_EVENTS_\w+) (\d+)", header))
    assert defines == {"UPKIE_EVENTS_SETTINGS_WORDS": str(abi.EVENTS_SETTINGS_WORDS), "UPKIE_EVENTS_LEVELS_MAX": str(abi.EVENTS_LEVELS_MAX)}
    section = header[header.index("---- Push curriculum"):header.index("#define UPKIE_EVENTS_SETTINGS_WORDS")]
    order = [section.index(word) for word in ("threshold uint32", "norm_min, norm_max float", "steps_min, steps_span uint32", "levels = L uint32",
                                              "up, down", "min_pushes uint32")]
    assert order == sorted(order), "the block's words are listed in the order of abi.EVENTS_SETTINGS"
    assert abi.EVENTS_SETTINGS == ("threshold", "norm_min", "norm_max", "steps_min", "steps_span", "levels", "up", "down", "min_pushes")
    table = {name: argtypes for name, _, argtypes, _ in lib._ABI}
    for name in ("upkie_sim_episode_events_step_levels", "upkie_sim_episode_events_reset_levels", "upkie_sim_episode_events_level_counts"):
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto is not None, name
        params = [p.strip() for p in proto.group(1).replace("\n", " ").split(",")]
        assert len(params) == len(table[name]), name
        for text, ctype in zip(params, table[name]):
            want = C.c_double if text.startswith("double ") else C.c_uint32 if text.startswith("uint32_t ") else C.c_void_p
            assert ctype is want, (name, text)
    # the old pair is declared as it was
    assert "int upkie_sim_episode_events_step(UpkieSim* sim, const UpkieEpisodeEvents* params, const uint8_t* terminated," in header


# ---------------------------------------------------------------- the library's refusals, without a device
@pytest.fixture(scope="module")
def library():
    lib.build()
    return lib.load()


def test_library_refuses_every_listed_limit_without_a_gpu(library):
    for name in ("upkie_sim_episode_events_step_levels", "upkie_sim_episode_events_reset_levels", "upkie_sim_episode_events_level_counts"):
        assert name in lib.EXPORTED_SYMBOLS and getattr(library, name) is not None
    err = lambda: library.upkie_sim_last_error(None)  # noqa: E731
    buf = (C.c_uint32 * 64)()
    state = [buf] * 8  # calls, remaining, pushes, episodes, level, episode_pushes, difficulty, force

    def step(variation=0.0, settings=buf, state=state, records=(None, None)):
        return library.upkie_sim_episode_events_step_levels(None, variation, settings, None, None, *state, *records, None)

    def reset(variation=0.0, settings=buf, state=state, records=(None, None), start=0):
        return library.upkie_sim_episode_events_reset_levels(None, variation, settings, start, None, *state, *records, None)

    for call in (step, reset):
        for variation in (-0.1, 1.0, float("nan")):
            assert call(variation=variation) == abi.ERR_INVALID_ARGUMENT and b"inertia_variation" in err(), (call.__name__, variation)
        # good settings and no handle, no block or a missing state buffer: a null argument, and never launched
        assert call() == abi.ERR_INVALID_ARGUMENT and b"null argument" in err()
        assert call(settings=None) == abi.ERR_INVALID_ARGUMENT and b"null argument" in err()
        for k in range(8):
            assert call(state=state[:k] + [None] + state[k + 1:]) == abi.ERR_INVALID_ARGUMENT and b"null argument" in err(), k
        # body_inertials / link_scale exactly when inertia_variation > 0
        for variation, records in ((0.3, (None, None)), (0.3, (buf, None)), (0.0, (buf, buf)), (0.0, (None, buf))):
            assert call(variation=variation, records=records) == abi.ERR_INVALID_ARGUMENT and b"exactly when inertia_variation > 0" in err()
        assert call(variation=0.3, records=(buf, buf)) == abi.ERR_INVALID_ARGUMENT and b"null argument" in err()
    assert reset(start=256) == abi.ERR_INVALID_ARGUMENT and b"start_level" in err()
    assert reset(start=255) == abi.ERR_INVALID_ARGUMENT and b"null argument" in err()  # (255 passes; the handle is what is missing)
    for args in ((None, buf, buf), (None, None, buf), (None, buf, None)):
        assert library.upkie_sim_episode_events_level_counts(*args, None) == abi.ERR_INVALID_ARGUMENT and b"null argument" in err()


# ---------------------------------------------------------------- the twin
@pytest.mark.parametrize("num_envs,offset", P.GPU_SIZES)
def test_with_one_level_the_twin_is_the_episode_events_twin_bit_for_bit(urdf_model, num_envs, offset):
    term, trunc = P.gpu_flags(num_envs, offset)
    kw = dict(seed=P.GPU_SEED, env_id_offset=offset, **P.GPU_SETTINGS)
    new, old = P.LevelTwin(urdf_model, num_envs, **kw), R.Twin(urdf_model, num_envs, **kw)
    for t in range(P.GPU_CALLS):
        a, b = new.step(term[t], trunc[t]), old.step(term[t], trunc[t])
        for name in b:
            assert np.array_equal(a[name], b[name]), (name, t)
        got, want = new.snapshot(), old.snapshot()
        for name in want:
            assert np.array_equal(got[name], want[name]), (name, t)
        assert not got["level"].any() and np.all(got["difficulty"] == 1.0)


def test_levels_stay_within_their_range_and_difficulty_is_their_fraction(urdf_model):
    for levels in (dict(levels=3, up=1, down=2), dict(levels=5, start=5, up=3, down=4), dict(levels=1, up=1, down=1), dict(levels=255, up=200, down=255)):
        twin = _twin(urdf_model, 65, 1000, **dict(dict(start=0, min_pushes=1), **levels))
        term, trunc = P.gpu_flags(65, 1000)
        seen = set()
        for t in range(P.GPU_CALLS):
            twin.step(term[t], trunc[t])
            assert twin.level.max() <= levels["levels"]
            assert np.array_equal(twin.difficulty, (twin.level.astype(np.float32) / np.float32(levels["levels"])).astype(np.float32))
            seen |= set(twin.level.tolist())
        assert 0 in seen and levels["levels"] in seen, (levels, sorted(seen))
    # a held difficulty: up = down = 0 leaves every env at its start
    twin = _twin(urdf_model, 65, 1000, levels=3, start=3, up=0, down=0)
    for t in range(P.GPU_CALLS):
        twin.step(term[t], trunc[t])
    assert np.all(twin.level == 3) and np.all(twin.difficulty == 1.0)


def test_a_level_is_invariant_to_batch_shard_and_an_id_offset_across_2_to_the_32(urdf_model):
    base = 2 ** 32 - 32  # envs 32-63 of the batch have ids beyond 2^32
    term, trunc = P.gpu_flags(64, base)
    whole = _trace(_twin(urdf_model, 64, base), term, trunc)
    assert max(s["level"].max() for s in whole) == 3
    for lo in (0, 32):
        shard = _trace(_twin(urdf_model, 32, base + lo), term[:, lo:lo + 32], trunc[:, lo:lo + 32])
        for a, b in zip(whole, shard):
            for name in a:
                assert np.array_equal(a[name][..., lo:lo + 32], b[name]), name
    # the other envs' flags: env 5 sees the same whatever envs 0-4 and 6-63 do
    other_term, other_trunc = P.gpu_flags(64, 77)
    other_term[:, 5], other_trunc[:, 5] = term[:, 5], trunc[:, 5]
    other = _trace(_twin(urdf_model, 64, base), other_term, other_trunc)
    assert any(not np.array_equal(a["level"], b["level"]) for a, b in zip(whole, other))
    for a, b in zip(whole, other):
        for name in a:
            assert np.array_equal(a[name][..., 5], b[name][..., 5]), name
    # and a level never changes which words an env draws: the schedule of starts is that of the plain stage while no push is held
    plain = R.Twin(urdf_model, 64, seed=P.GPU_SEED, env_id_offset=base, **dict(P.GPU_SETTINGS, push_steps=(1, 1)))
    level = _twin(urdf_model, 64, base, push_steps=(1, 1))
    for t in range(P.GPU_CALLS):
        assert np.array_equal(plain.step(term[t], trunc[t])["start"], level.step(term[t], trunc[t])["start"])
    assert np.array_equal(plain.pushes, level.pushes) and not np.array_equal(plain.force, level.force)


# ---------------------------------------------------------------- the GPU test's inputs
def test_the_gpu_tests_inputs_meet_every_branch(urdf_model):
    seen = {name: 0 for name in P.BRANCHES}
    starts = np.zeros(P.GPU_LEVELS["levels"] + 1, dtype=int)
    both = 0

    def watch(happened):
        for name in seen:
            seen[name] += int(happened[name].sum())
        starts[:] += np.bincount(happened["start_level"][happened["start_level"] >= 0], minlength=len(starts))

    for num_envs, offset in P.GPU_SIZES:
        term, trunc = P.gpu_flags(num_envs, offset)
        both += int((term & trunc).sum())
        _trace(_twin(urdf_model, num_envs, offset), term, trunc, watch)
    print(seen, "starts per level", starts.tolist(), "ends with both flags", both)
    assert all(seen.values()), seen
    assert starts.all(), starts
    assert both > 0, "terminated wins when both flags are set: some end has to carry both"


def test_the_interpolated_top_misses_the_exact_one_at_the_gpu_tests_norms():
    lo, hi = np.float32(P.NORM_MIN), np.float32(P.NORM_MAX)
    assert float(lo) == P.NORM_MIN and float(hi) == P.NORM_MAX, "the norms are float32 numbers: the block holds them exactly"
    top = np.array([3])
    assert P.norm_high(top, 3, P.NORM_MIN, P.NORM_MAX)[0] == P.NORM_MAX
    assert P.norm_high(top, 3, P.NORM_MIN, P.NORM_MAX, interpolate_top=True)[0] == float(np.nextafter(hi, np.float32(0.0)))
    assert np.array_equal(P.norm_high(np.array([0, 0]), 3, P.NORM_MIN, P.NORM_MAX), [P.NORM_MIN] * 2)
    assert np.array_equal(P.norm_high(np.array([0]), 0, 5.0, 20.0), [20.0]), "L = 0: the top, no division"
    assert P.difficulty_of(np.array([0, 1, 2, 3, 9]), 3).tolist() == [0.0, np.float32(1) / np.float32(3), np.float32(2) / np.float32(3), 1.0, 1.0]


@pytest.mark.parametrize("num_envs,offset", P.GPU_SIZES[1:])  # (one env alone cannot meet every case in 40 calls: the five larger batches each do)
def test_the_gpu_tests_inputs_tell_five_bugs_from_the_stage(urdf_model, num_envs, offset):
    term, trunc = P.gpu_flags(num_envs, offset)
    trace = _trace(_twin(urdf_model, num_envs, offset), term, trunc)
    assert len(P.MUTATIONS) == 5
    for mutation in P.MUTATIONS:
        mutant = _trace(_twin(urdf_model, num_envs, offset, mutation=mutation), term, trunc)
        differs = any(not np.array_equal(a[name], b[name]) for a, b in zip(trace, mutant) for name in a)
        assert differs, mutation


# ---------------------------------------------------------------- Ppo's call order under a levelled events object
class _LevelEvents:
    """What `Ppo` and `AgentStep` use of an `EpisodeEvents` with a curriculum, recorded."""

    def __init__(self, calls):
        self.calls, self.num_envs = calls, N
        self.curriculum, self.live = PushLevels(3), True

    def reset(self):
        self.calls.add("events.reset")

    def step(self, terminated, truncated):
        self.calls.add("events.step", terminated=terminated, truncated=truncated)

    def log(self):
        self.calls.add("events.log")
        return {"push_level_mean": 1.5, "push_level_top_frac": 0.25, "push_prob": 0.5, "push_norm_high": 20.0}


@pytest.mark.parametrize("pipeline,normalizer,reward", [(False, True, "terms"), (True, True, "fn"), (False, False, "env")])
def test_ppos_call_order_is_unchanged_with_levelled_events(pipeline, normalizer, reward):
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    calls = Calls()
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=N, frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=4,
                   sim_factory=oracle_sim_factory) as inner:
        events = _LevelEvents(calls)
        model = _model(Env(inner, calls), calls, pipeline, normalizer, reward, events=events)
        assert model.events is events and model._agent.events is events
        reset = inner.reset(seed=0)
        model._obs = reset[0] if isinstance(reset, tuple) else reset
        model.collect_rollouts()
    per_step = [name for name in calls.names[:-2] if name != "events.step"]
    assert per_step == STEP_CALLS[(pipeline, normalizer, reward)] * T, "every other stage is called as without events"
    assert calls.names[-2:] == ["value", "gae"] and "events.log" not in calls.names and "events.reset" not in calls.names
    # the stage is stepped once per env step, after the reward and before the statistics, with the env's own flag tensors
    before = {"terms": "reward.step", "fn": "reward_fn", "env": "env.step"}[reward]
    where = [i for i, name in enumerate(calls.names) if name == "events.step"]
    assert len(where) == T and all(calls.names[i - 1] == before and calls.names[i + 1] == "episodes" for i in where)
    for k in range(T):
        out = calls.args["env.step"][k]["out"]
        assert calls.args["events.step"][k]["terminated"] is out[2] and calls.args["events.step"][k]["truncated"] is out[3]
    assert D == 4
