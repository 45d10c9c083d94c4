"""The evaluation tally without a GPU: the twins of tests/evaluation_reference.py against each other, the numpy model of
the kernel's order and its mutations, the refusals of the new entry points, and `EvalCallback`'s bookkeeping against
fakes."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import evaluation_reference as R
from upkie_amd import abi, lib
from upkie_amd.evaluation import EvalCallback, EpisodeTally, PolicyEvaluator, evaluate_policy
from upkie_amd.exceptions import UpkieRuntimeError
from upkie_amd.ppo import Ppo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("upkie_eval_workspace_bytes", "upkie_eval_reset", "upkie_eval_step")
SMALL = [r for r in R.EVAL_ROWS if r.N <= 5000]


@pytest.fixture(scope="module")
def library():
    lib.build()
    return lib.load()


# ---------------------------------------------------------------- the twins
@pytest.mark.parametrize("N,E", R.TARGET_TABLE)
def test_the_quotas_sum_to_the_episodes_asked_for(N, E):
    t = R.targets(N, E)
    assert int(t.sum()) == E and t.min() >= 0 and t.max() - t.min() <= 1
    assert all(a <= b for a, b in zip(t[:-1], t[1:])), "the later envs give the extra episodes"
    if N > E:
        assert t[:N - E].tolist() == [0] * (N - E) and t[N - E:].tolist() == [1] * E, "only the last E envs count"
    assert np.array_equal(R.EvalOrderModel(N, E).target, t)


@pytest.mark.parametrize("row", R.EVAL_ROWS, ids=R.EVAL_IDS)
def test_every_rows_script_fills_the_quota_on_the_twin(row):
    """A GPU test can never pass by comparing two unfinished tallies; and the rows are what they claim."""
    script = R.eval_script(row)
    twin = R.BatchEvaluateTwin(row.N, row.E)
    fills = []
    R.run_eval_script(script, twin, after=lambda t: fills.append(twin.filled))
    assert fills[0] == 0 and fills[-1] == row.E and twin.steps <= R.EVAL_STEPS
    assert np.array_equal(twin.count, twin.target)
    if row.E >= 64:
        assert 0 < fills[1] < fills[3] < row.E, "the list is part full behind the random steps"
    assert not script.terminated[0].any() and not script.truncated[0].any()
    assert script.terminated[5].all() and script.truncated[5, ::2].all() and not script.truncated[5, 1::2].any()
    done1 = script.terminated[1] | script.truncated[1]
    assert done1[-1] and done1.sum() == 1


def test_the_rows_reach_the_geometries_they_claim():
    plan = {(r.N, r.E): R.episodes_blocks(r.N) for r in R.EVAL_ROWS}
    assert plan[(257, 300)] == (2, 129)
    assert plan[(4099, 1025)][0] == 17 and -(-1025 // R.EVAL_STAGE) == 2 and 1025 % R.EVAL_STAGE == 1
    blocks, rows = plan[(65537, 70000)]
    assert blocks == 257 and 65537 - (blocks - 1) * rows == 1
    blocks, rows = plan[(262145, 262145)]
    assert rows == 257 and R.episodes_blocks(262144)[1] == 256
    assert sorted(set(R.targets(65, 200).tolist())) == [3, 4]


@pytest.mark.parametrize("row", SMALL, ids=[f"N{r.N}-E{r.E}" for r in SMALL])
def test_the_batched_twin_is_the_python_loop(row):
    script = R.eval_script(row)
    loop, batch = R.EvaluateTwin(row.N, row.E), R.BatchEvaluateTwin(row.N, row.E)

    def look(t):
        for name in ("rec_return", "rec_length", "rec_env", "rec_truncated", "steps"):
            assert getattr(loop, name) == getattr(batch, name), (name, t)
        assert np.array_equal(loop.count, batch.count)
        for a, b in zip(loop.running(), batch.running()):
            assert np.array_equal(a, b)

    R.run_eval_script(script, loop, batch, after=look)
    assert loop.summary() == batch.summary()


@pytest.mark.parametrize("row", SMALL, ids=[f"N{r.N}-E{r.E}" for r in SMALL])
def test_the_order_model_is_the_twin_bit_for_bit(row):
    script = R.eval_script(row)
    model, twin = R.EvalOrderModel(row.N, row.E), R.EvaluateTwin(row.N, row.E)
    R.run_eval_script(script, model, twin, after=lambda t: pytest.fail(f"step {t}") if not R.same_as_twin(model, twin) else None)
    assert model.filled == row.E and model.summary == twin.summary()


@pytest.mark.parametrize("mutation", R.EVAL_MUTATIONS)
def test_every_mutation_of_the_order_model_differs_from_the_twin(mutation):
    differs = {}
    for row in (R.EvalRow(257, 300, ""), R.EvalRow(4099, 1025, "")):
        script = R.eval_script(row)
        model, twin = R.EvalOrderModel(row.N, row.E, mutation=mutation), R.EvaluateTwin(row.N, row.E)
        seen = []
        R.run_eval_script(script, model, twin, after=lambda t: seen.append(R.same_as_twin(model, twin)))
        differs[row.N] = not all(seen)
    assert all(differs.values()), differs


@pytest.mark.parametrize("row", SMALL, ids=[f"N{r.N}-E{r.E}" for r in SMALL])
def test_the_sequential_summary_agrees_with_numpy(row):
    twin = R.EvaluateTwin(row.N, row.E)
    R.run_eval_script(R.eval_script(row), twin)
    mean_r, var_r, mean_l, var_l, lo, hi, frac = twin.summary()
    r, l = np.array(twin.rec_return), np.array(twin.rec_length, dtype=np.float64)
    assert mean_r == pytest.approx(np.mean(r), rel=1e-12)
    assert np.sqrt(var_r) == pytest.approx(np.std(r), rel=1e-12, abs=1e-300)
    assert mean_l == pytest.approx(np.mean(l), rel=1e-12) and np.sqrt(var_l) == pytest.approx(np.std(l), rel=1e-12, abs=1e-300)
    assert lo == r.min() and hi == r.max() and frac == np.mean(twin.rec_truncated)


# ---------------------------------------------------------------- the C-ABI
def test_the_symbols_are_declared_listed_and_exported(library):
    with open(os.path.join(ROOT, "include", "upkie_hip.h")) as f:
        declared = set(re.findall(r"\b(upkie_[a-z_]+)\s*\(", f.read()))
    for name in SYMBOLS:
        assert name in declared and name in lib.EXPORTED_SYMBOLS and getattr(library, name) is not None
    assert any(s.endswith("eval_episodes.hpp") for s in lib.SOURCES)


def _step_args(N, capacity, E, null=None):
    """Arguments of upkie_eval_step over host buffers (never read: the refusals come before any device use)."""
    keep = [np.zeros(max(N, capacity, 1) * 2 + 1024, dtype=np.float64) for _ in range(14)]
    names = ("reward", "terminated", "truncated", "ep_return", "ep_length", "count", "target", "rec_return", "rec_length", "rec_env",
             "rec_truncated", "counters", "summary", "workspace")
    ptrs = [None if n == null else a.ctypes.data for n, a in zip(names, keep)]
    return keep, [N, capacity, E] + ptrs + [None]


def _message(library):
    return library.upkie_sim_last_error(None).decode()


def test_the_entry_points_refuse_bad_arguments_without_a_device(library):
    import torch

    bad = abi.ERR_INVALID_ARGUMENT
    for N in (0, -3):
        assert library.upkie_eval_workspace_bytes(N) == bad and "num_envs" in _message(library)
    assert library.upkie_eval_workspace_bytes(37) == 256 + 4096 + 37 * 17
    for N, cap, E, word in ((0, 8, 4, "num_envs"), (8, 0, 1, "capacity"), (8, 8, 0, "n_eval_episodes"), (8, 8, -1, "n_eval_episodes"),
                            (8, 8, 9, "n_eval_episodes")):
        keep, args = _step_args(N, cap, E)
        assert library.upkie_eval_step(*args) == bad and word in _message(library), (N, cap, E)
        assert library.upkie_eval_reset(*(args[:3] + args[6:10] + args[14:16] + [None])) == bad and word in _message(library), (N, cap, E)
    for name in ("reward", "ep_return", "ep_length", "count", "target", "rec_return", "rec_length", "rec_env", "rec_truncated", "counters", "summary",
                 "workspace"):
        keep, args = _step_args(8, 8, 4, null=name)
        assert library.upkie_eval_step(*args) == bad and "null" in _message(library), name
    for name in ("ep_return", "ep_length", "count", "target", "counters", "summary"):
        keep, args = _step_args(8, 8, 4, null=name)
        assert library.upkie_eval_reset(*(args[:3] + args[6:10] + args[14:16] + [None])) == bad and "null" in _message(library), name
    if not torch.cuda.is_available():  # good arguments: refused for the lack of a device, nothing computed elsewhere
        keep, args = _step_args(8, 8, 4, null="terminated")
        assert library.upkie_eval_step(*args) == abi.ERR_NO_DEVICE
        assert library.upkie_eval_reset(*(args[:3] + args[6:10] + args[14:16] + [None])) == abi.ERR_NO_DEVICE
        with pytest.raises(UpkieRuntimeError):
            EpisodeTally(8, 8, device="cpu")


def test_the_python_objects_refuse_bad_sizes_before_any_device_use():
    for N, cap in ((0, 4), (4, 0)):
        with pytest.raises(ValueError):
            EpisodeTally(N, cap)

    class Env:
        num_envs, autoreset_mode, max_episode_steps = 8, "next_step", 20

    with pytest.raises(ValueError, match="same_step"):
        evaluate_policy(object(), Env(), n_eval_episodes=4)
    Env.autoreset_mode = "disabled"
    with pytest.raises(ValueError, match="same_step"):
        PolicyEvaluator(object(), Env(), 4)
    for kw in (dict(n_eval_episodes=0), dict(eval_freq=0)):
        with pytest.raises(ValueError):
            EvalCallback(Env(), **kw)


# ---------------------------------------------------------------- EvalCallback's bookkeeping
class _FakeEnv:
    num_envs = 8


class _FakeTrainer:
    def set_progress(self, p):
        pass

    def log(self):
        return {"loss": 1.0}


class _FakeEpisodes:
    def ep_rew_mean(self):
        return 2.5

    def ep_len_mean(self):
        return None


class _BookkeepingPpo(Ppo):
    """`Ppo.learn` around stages that count: 8 envs x 4 steps = 32 timesteps an iteration."""

    saved = None

    def _setup(self):
        if self.trainer is None:
            self.trainer, self.episodes, self.saved = _FakeTrainer(), _FakeEpisodes(), []

    def collect_rollouts(self):
        self.num_timesteps += self.n_steps * self.n_envs

    def train(self):
        pass

    def save(self, path):
        self.saved.append((path, self.iterations))


class _ScriptedCallback(EvalCallback):
    """`EvalCallback` whose evaluations give the means of a script, in turn."""

    def __init__(self, means, **kw):
        super().__init__(object(), **kw)
        self.means, self.evaluated_at = list(means), []

    def evaluate(self, model):
        self.evaluated_at.append(model.iterations)
        mean = self.means[len(self.evaluated_at) - 1]
        return {"mean_reward": mean, "std_reward": 0.5, "mean_ep_length": 20.0, "std_ep_length": 0.0, "min_reward": mean, "max_reward": mean,
                "time_limit_frac": 0.25, "episode_rewards": [mean] * self.n_eval_episodes, "episode_lengths": [20] * self.n_eval_episodes,
                "episode_envs": list(range(self.n_eval_episodes))}


EVAL_KEYS = {"eval/mean_reward", "eval/mean_ep_length", "eval/time_limit_frac"}


@pytest.mark.parametrize("eval_freq,want", [(4, [1, 2, 3, 4, 5, 6]), (8, [2, 4, 6]), (10, [3, 5]), (12, [3, 6]), (5, [2, 3, 4, 5]), (100, [])])
def test_the_callback_evaluates_at_the_first_iteration_at_or_after_each_multiple(eval_freq, want):
    """Iteration k ends at vec-env step 4 k; eval_freq counts vec-env steps, as SB3's n_calls."""
    cb = _ScriptedCallback([1.0] * 6, eval_freq=eval_freq, n_eval_episodes=3)
    model = _BookkeepingPpo(_FakeEnv(), object(), n_steps=4)
    model.learn(6 * 32, callback=cb)
    assert model.iterations == 6, "the callback returns nothing that stops training"
    assert cb.evaluated_at == want
    assert cb.evaluations["timesteps"] == [32 * k for k in want]
    for rec in model.records:
        assert bool(EVAL_KEYS & rec.keys()) == (rec["time/iterations"] in want)
        assert not (EVAL_KEYS & rec.keys()) or EVAL_KEYS <= rec.keys()


def test_the_callback_keeps_the_best_and_saves_only_on_improvement():
    means = [1.0, 3.0, 2.0, 3.0, 4.0, -1.0]
    cb = _ScriptedCallback(means, eval_freq=4, n_eval_episodes=2, best_model_save_path="best.pt")
    model = _BookkeepingPpo(_FakeEnv(), object(), n_steps=4)
    returned = []
    model.learn(6 * 32, callback=lambda m, rec: returned.append(cb(m, rec)))
    assert returned == [None] * 6
    assert model.saved == [("best.pt", 1), ("best.pt", 2), ("best.pt", 5)], "a tie is no improvement"
    assert cb.best_mean_reward == 4.0 and cb.last_mean_reward == -1.0
    assert cb.evaluations["results"] == [[m, m] for m in means] and cb.evaluations["ep_lengths"] == [[20, 20]] * 6
    assert [rec["eval/mean_reward"] for rec in model.records] == means
    assert model.records[0] == {"train/loss": 1.0, "rollout/ep_rew_mean": 2.5, "rollout/ep_len_mean": None, "time/total_timesteps": 32,
                                "time/iterations": 1, "eval/mean_reward": 1.0, "eval/mean_ep_length": 20.0, "eval/time_limit_frac": 0.25}
    # without a path nothing is saved
    cb = _ScriptedCallback(means, eval_freq=4, n_eval_episodes=2)
    model = _BookkeepingPpo(_FakeEnv(), object(), n_steps=4)
    model.learn(6 * 32, callback=cb)
    assert model.saved == [] and cb.best_mean_reward == 4.0


def test_off_the_log_interval_the_callback_makes_its_own_record():
    cb = _ScriptedCallback([1.0, 2.0, 3.0], eval_freq=8, n_eval_episodes=2)
    model = _BookkeepingPpo(_FakeEnv(), object(), n_steps=4)
    model.learn(6 * 32, callback=cb, log_interval=4)  # records at iteration 4 alone; evaluations at 2, 4, 6
    assert [rec["time/iterations"] for rec in model.records] == [2, 4, 6]
    assert model.records[0] == {"time/total_timesteps": 64, "time/iterations": 2, "eval/mean_reward": 1.0, "eval/mean_ep_length": 20.0,
                                "eval/time_limit_frac": 0.25}
    assert "train/loss" in model.records[1] and model.records[1]["eval/mean_reward"] == 2.0
    # a second learn() that restarts the count evaluates from the first multiple again
    cb2 = _ScriptedCallback([7.0, 8.0, 9.0], eval_freq=8, n_eval_episodes=2)
    model.learn(4 * 32, callback=cb2)
    model.learn(2 * 32, callback=cb2)
    assert cb2.evaluated_at == [2, 4, 2]


def test_a_restarted_learn_of_the_same_length_is_seen_as_a_restart():
    """Two runs of one iteration each end at the same vec-env step: the second still evaluates (the iteration count, not the
    step count, says that `learn` started over); a continued run (reset_num_timesteps=False) goes on counting."""
    cb = _ScriptedCallback([1.0, 2.0, 3.0, 4.0], eval_freq=4, n_eval_episodes=2)
    model = _BookkeepingPpo(_FakeEnv(), object(), n_steps=4)
    model.learn(32, callback=cb)
    model.learn(32, callback=cb)
    assert cb.evaluated_at == [1, 1] and cb.evaluations["timesteps"] == [32, 32]
    model.learn(64, callback=cb, reset_num_timesteps=False)
    assert cb.evaluated_at == [1, 1, 2, 3] and cb.evaluations["timesteps"] == [32, 32, 64, 96]
