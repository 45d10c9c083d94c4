"""The push curriculum on the MI355X: the levelled launch against the fp64 twin (tests/push_curriculum_reference.py) call by
call, with one level against the plain launch bit for bit, sharding and reset device against device, a captured loop that
follows `set_push` and `set_levels`, the level histogram, and `Ppo` with levelled events: graphed against eager, save /
load, the record's fields, an `EvalCallback` at the top level that leaves training alone, the example."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import push_curriculum_reference as P
from tests.training_rig import (bits, check_event_records, events_stage, pendulum, pitch_reward, read_state, same, snapshot, tower,
                                warm_up_as_the_capture_does)
from upkie_amd import abi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_NORM = P.GPU_SETTINGS["push_norm"][1]
INTEGERS = ("calls", "remaining", "pushes", "episodes", "level", "episode_pushes")


@pytest.fixture(scope="module")
def model():
    from upkie_amd.model.model import Model

    return Model()


def _stage(model, num_envs, offset, levels=P.GPU_LEVELS, settings=P.GPU_SETTINGS, **kw):
    from upkie_amd.events import PushLevels

    if levels is not None:
        kw["curriculum"] = PushLevels(**levels)
    return events_stage(model, num_envs, offset, P.GPU_SEED, **dict(settings, **kw))


def _flags(num_envs, offset, device):
    term, trunc = P.gpu_flags(num_envs, offset)
    return term, trunc, torch.from_numpy(term).to(device), torch.from_numpy(trunc).to(device)


def _integers_equal(got, want, where):
    for name in INTEGERS:
        assert np.array_equal(bits(got[name]), bits(want[name].astype(np.uint32) if name != "remaining" else want[name])), (name, where)
    assert np.array_equal(bits(got["difficulty"]), bits(want["difficulty"])), ("difficulty", where)


@pytest.mark.parametrize("num_envs,offset", P.GPU_SIZES)
def test_the_levelled_kernel_is_the_twin_after_every_call(model, num_envs, offset):
    sim, events = _stage(model, num_envs, offset)
    twin = P.LevelTwin(model.struct, num_envs, seed=P.GPU_SEED, env_id_offset=offset, **P.GPU_LEVELS, **P.GPU_SETTINGS)
    assert sim.ext_force.data_ptr() == events.force.data_ptr() and sim.body_inertials.data_ptr() == events.body_inertials.data_ptr()
    term, trunc, d_term, d_trunc = _flags(num_envs, offset, sim.device)
    every = np.arange(num_envs)
    prev = read_state(events)
    assert set(prev) == set(INTEGERS) | {"force", "body_inertials", "link_scale", "settings", "difficulty"}
    check_event_records(prev, twin.snapshot(), every)  # construction: episode 0
    _integers_equal(prev, twin.snapshot(), "construction")
    worst_force, starts = 0.0, 0
    for t in range(P.GPU_CALLS):
        events.step(d_term[t], d_trunc[t])
        happened = twin.step(term[t], trunc[t])
        got, want = read_state(events), twin.snapshot()
        _integers_equal(got, want, t)
        assert np.array_equal(bits(got["difficulty"]), bits(P.difficulty_of(got["level"].astype(np.int64), P.GPU_LEVELS["levels"])))
        force, before = got["force"][0], prev["force"][0]
        assert np.all(bits(force[:, happened["zero"]]) == 0), "a free step without a start: +0.0 in every word"
        assert np.array_equal(bits(force[:, happened["hold"]]), bits(before[:, happened["hold"]])), "a held force is not written"
        s = happened["start"]
        if s.any():
            worst_force = max(worst_force, float(np.abs(force[:, s].astype(np.float64) - want["force"][:, s]).max()))
            starts += int(s.sum())
        done = happened["redrawn"]
        if done.any():
            check_event_records(got, want, np.flatnonzero(done))
        for name in ("body_inertials", "link_scale"):
            assert np.array_equal(bits(got[name][:, ~done]), bits(prev[name][:, ~done])), f"{name} of envs that did not end is not written"
        assert np.array_equal(bits(got["settings"]), bits(prev["settings"])), "the block is read, never written"
        prev = got
    print(f"N = {num_envs}, offset {offset}: {starts} starts, worst |force - twin| {worst_force:.3g} N (bound {2.5e-6 * MAX_NORM:.3g})")
    assert worst_force < 2.5e-6 * MAX_NORM
    sim.close()


@pytest.mark.parametrize("num_envs,offset", P.GPU_SIZES)
def test_with_one_level_the_new_entry_point_leaves_the_bits_of_the_old_one(model, num_envs, offset):
    sim_a, old = _stage(model, num_envs, offset, levels=None)
    sim_b, new = _stage(model, num_envs, offset, levels=None, live=True)
    assert old.settings is None and new.settings is not None and new.curriculum is None
    term, trunc, d_term, d_trunc = _flags(num_envs, offset, sim_a.device)
    for t in range(P.GPU_CALLS):
        old.step(d_term[t], d_trunc[t])
        new.step(d_term[t], d_trunc[t])
        a, b = read_state(old), read_state(new)
        assert set(b) - set(a) == {"settings", "level", "episode_pushes", "difficulty"}
        for name in a:
            assert np.array_equal(bits(a[name]), bits(b[name])), (name, t)
        assert not b["level"].any() and np.all(b["difficulty"] == 1.0)
    assert a["pushes"].sum() > 0 or num_envs == 1
    sim_a.close()
    sim_b.close()


def test_one_levelled_handle_of_64_is_two_of_32_bit_for_bit(model):
    term, trunc = P.gpu_flags(64, 0)

    def run(num_envs, offset, lo):
        sim, events = _stage(model, num_envs, offset)
        d_term = torch.from_numpy(np.ascontiguousarray(term[:, lo:lo + num_envs])).to(sim.device)
        d_trunc = torch.from_numpy(np.ascontiguousarray(trunc[:, lo:lo + num_envs])).to(sim.device)
        trace = []
        for t in range(P.GPU_CALLS):
            events.step(d_term[t], d_trunc[t])
            trace.append(read_state(events))
        sim.close()
        return trace

    whole = run(64, 0, 0)
    assert whole[-1]["level"].max() == 3 and whole[-1]["level"].min() == 0
    for lo in (0, 32):
        for a, b in zip(whole, run(32, lo, lo)):
            for name in a:
                sl = a[name] if name == "settings" else a[name][..., lo:lo + 32]
                assert np.array_equal(bits(sl), bits(b[name])), name


def test_a_masked_reset_restarts_only_its_envs_at_the_start_level(model):
    N, offset = 65, 1000
    sim, events = _stage(model, N, offset, levels=dict(P.GPU_LEVELS, start=1))
    term, trunc, d_term, d_trunc = _flags(N, offset, sim.device)
    first = read_state(events)
    assert np.all(first["level"] == 1) and np.all(first["difficulty"] == np.float32(1) / np.float32(3))
    for t in range(12):
        events.step(d_term[t], d_trunc[t])
    moved = read_state(events)
    assert len(set(moved["level"].tolist())) >= 3 and moved["episode_pushes"].max() >= 1 and np.all(moved["calls"] == 12)
    mask = np.zeros(N, dtype=np.uint8)
    mask[::3] = 1
    events.reset(torch.from_numpy(mask).to(sim.device))
    got, m = read_state(events), mask.astype(bool)
    for name in ("calls", "remaining", "pushes", "episodes", "episode_pushes"):
        assert np.all(got[name][m] == 0), name
    assert np.all(got["level"][m] == 1) and np.all(got["difficulty"][m] == np.float32(1) / np.float32(3)) and np.all(bits(got["force"][0][:, m]) == 0)
    for name in got:
        if name != "settings":
            assert np.array_equal(bits(got[name][..., ~m]), bits(moved[name][..., ~m])), name
    for name in ("body_inertials", "link_scale"):  # (the masked envs: the records of episode 0 again)
        assert np.array_equal(bits(got[name][:, m]), bits(first[name][:, m])), name
    events.reset()
    again = read_state(events)
    for name in first:
        assert np.array_equal(bits(again[name]), bits(first[name])), name
    sim.close()


def test_a_captured_loop_follows_set_push_and_set_levels(model):
    """Four steps in one hipGraph, replayed; between replays the block and the levels are rewritten from outside. The
    eager twin makes the same changes at the same calls."""
    N, offset, K = 65, 1000, 4
    sim, events = _stage(model, N, offset)
    twin = P.LevelTwin(model.struct, N, seed=P.GPU_SEED, env_id_offset=offset, **P.GPU_LEVELS, **P.GPU_SETTINGS)
    term, trunc, _, _ = _flags(N, offset, sim.device)
    d_term, d_trunc = (torch.zeros((K, N), dtype=torch.uint8, device=sim.device) for _ in range(2))
    events.step(d_term[0], d_trunc[0])  # (warm-up off the capture, undone by the reset)
    events.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(K):
            events.step(d_term[k], d_trunc[k])
    events.reset()  # (the capture launched nothing, but says so)
    changes = {
        1: lambda s: s.set_push(prob=0.6, norm=(2.0, 30.0)),
        2: lambda s: s.set_levels(2),
        3: lambda s: s.set_push(steps=(2, 4)),
        4: lambda s: s.set_levels(torch.arange(N, dtype=torch.int32) % 4 if s is events else np.arange(N) % 4),
        5: lambda s: s.set_push(prob=0.05),
    }
    worst = 0.0
    for replay in range(6):
        if replay in changes:
            changes[replay](events)
            changes[replay](twin)
        rows = slice(replay * K, (replay + 1) * K)
        d_term.copy_(torch.from_numpy(term[rows]))
        d_trunc.copy_(torch.from_numpy(trunc[rows]))
        graph.replay()
        for t in range(rows.start, rows.stop):
            twin.step(term[t], trunc[t])
        got, want = read_state(events), twin.snapshot()
        _integers_equal(got, want, replay)
        worst = max(worst, float(np.abs(got["force"][0].astype(np.float64) - want["force"]).max()))
    print(f"worst |force - twin| over the replays {worst:.3g} N (bound {2.5e-6 * 30.0:.3g})")
    assert worst < 2.5e-6 * 30.0
    assert events.push_prob == 0.05 and events.push_norm == (2.0, 30.0) and events.push_steps == (2, 4)
    assert events.log() == {"push_level_mean": float(got["level"].sum()) / N, "push_level_top_frac": float((got["level"] == 3).sum()) / N}
    with pytest.raises(ValueError, match="push_norm"):
        events.set_push(norm=(3.0, 2.0))
    with pytest.raises(ValueError, match="levels must be in 0-3"):
        events.set_levels(4)
    with pytest.raises(ValueError, match="levels must be in 0-3"):
        events.set_levels(torch.full((N,), 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="integer tensor"):
        events.set_levels(torch.zeros(N + 1, dtype=torch.int32))
    assert np.array_equal(bits(read_state(events)["settings"]), bits(got["settings"])), "a refused change writes nothing"
    sim.close()


def test_a_plain_stage_refuses_the_calls_that_need_a_block(model):
    from upkie_amd.exceptions import UpkieRuntimeError

    sim, plain = _stage(model, 4, 0, levels=None)
    for name, args in (("set_push", dict(prob=0.5)), ("set_levels", dict(levels=0)), ("level_counts", {})):
        with pytest.raises(UpkieRuntimeError, match=f"{name} needs the push settings in a device block"):
            getattr(plain, name)(**args)
    assert plain.log() == {} and set(plain.state_tensors()) == {"calls", "remaining", "pushes", "episodes", "force", "body_inertials", "link_scale"}
    sim.close()


@pytest.mark.parametrize("num_envs", (1, 65, 257, 70001))
def test_level_counts_is_numpys_bincount(model, num_envs):
    sim, events = _stage(model, num_envs, 0, levels=dict(levels=255, start=0, up=1, down=1), settings=dict(push_prob=0.25))
    rng = np.random.default_rng(num_envs)
    for high in (256, 3):  # (every bin in use; then a few crowded ones)
        levels = rng.integers(0, high, size=num_envs)
        events.set_levels(torch.from_numpy(levels.astype(np.int32)))
        counts = events.level_counts()
        assert counts.dtype == torch.int32 and tuple(counts.shape) == (256,) and counts.is_cuda
        assert np.array_equal(counts.cpu().numpy(), np.bincount(levels, minlength=256)), high
    assert np.array_equal(events.level_counts().cpu().numpy(), np.bincount(levels, minlength=256)), "a second call starts from zero"
    sim.close()


# ---------------------------------------------------------------- Ppo
B, T = 64, 8
EVENT_KEYS = ("events.calls", "events.remaining", "events.pushes", "events.episodes", "events.force", "events.body_inertials", "events.link_scale")
SETTINGS = dict(push_prob=0.3, push_norm=(5.0, 20.0), push_steps=(1, 3), inertia_variation=0.2)
LEVELS = dict(levels=3, start=1, up=1, down=2, min_pushes=1)
LEVEL_KEYS = ("events.settings", "events.level", "events.episode_pushes", "events.difficulty")


def _make(**kw):
    from upkie_amd.events import EpisodeEvents, PushLevels
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.ppo import Ppo

    torch.manual_seed(0)
    env = pendulum(B, 5, seed=0)
    dev = env.device
    policy = MlpActorCritic.from_modules(tower(4, 1).to(dev), tower(4, 1).to(dev), torch.nn.Parameter(torch.zeros(1, device=dev)),
                                         action_low=[-1.0], action_high=[1.0], seed=0)
    events = EpisodeEvents(env, curriculum=PushLevels(**LEVELS), live=True, **SETTINGS)
    model = Ppo(env, policy, n_steps=T, n_epochs=2, batch_size=B * T // 2, seed=0, reward_fn=pitch_reward, events=events, **kw)
    return env, policy, model


def _harder_after_the_first(m, record):
    if m.iterations == 1:
        m.events.set_push(prob=0.6, norm=(5.0, 25.0))


def test_ppo_with_levelled_events_graphed_equals_not_graphed_and_records_the_levels():
    env, policy, model = _make(graph=True)
    with env:
        model.learn(3 * B * T, callback=_harder_after_the_first)
        graphed = snapshot(model)
    env, policy, model = _make(graph=False)
    with env:
        warm_up_as_the_capture_does(model)
        model.learn(3 * B * T, callback=_harder_after_the_first)
        eager = snapshot(model)
    assert all(k in graphed[0] for k in EVENT_KEYS + LEVEL_KEYS + ("packed", "m", "v"))
    for k in graphed[0]:
        assert same(graphed[0][k], eager[0][k]), k
    assert same(graphed[1], eager[1]) and len(graphed[1]) == 3
    level = graphed[0]["events.level"].cpu().numpy()
    first, last = graphed[1][0], graphed[1][-1]
    assert level.max() == 3 and first["rollout/push_level_mean"] < last["rollout/push_level_mean"], "the levels moved inside the captured rollout"
    assert last["rollout/push_level_mean"] == float(level.sum()) / B and last["rollout/push_level_top_frac"] == float((level == 3).sum()) / B
    # (the block holds the probability as a 24-bit threshold)
    assert [round(r["rollout/push_prob"] * 2 ** 24) for r in graphed[1]] == [round(0.3 * 2 ** 24)] + [round(0.6 * 2 ** 24)] * 2
    assert [r["rollout/push_norm_high"] for r in graphed[1]] == [20.0, 25.0, 25.0]
    assert all("train/loss" in r and "rollout/ep_rew_mean" in r for r in graphed[1])


def test_ppo_with_levelled_events_resumes_bit_for_bit(tmp_path):
    from upkie_amd.ppo import Ppo

    path = str(tmp_path / "ppo.pt")
    env, policy, model = _make(graph=True)
    with env:
        model.learn(2 * B * T, callback=_harder_after_the_first)
        whole = snapshot(model)
    env, policy, model = _make(graph=True)
    with env:
        model.learn(2 * B * T, callback=lambda m, rec: (_harder_after_the_first(m, rec), m.iterations < 1)[1])
        assert model.iterations == 1
        model.save(path)
    saved = torch.load(path, map_location="cpu", weights_only=True)["tensors"]
    assert all(k in saved for k in LEVEL_KEYS) and saved["events.level"].dtype == torch.int32
    env, policy, fresh = _make(graph=True)
    with env:
        resumed = Ppo.load(path, env, policy, n_steps=T, n_epochs=2, batch_size=B * T // 2, seed=0, reward_fn=pitch_reward, events=fresh.events)
        assert torch.equal(fresh.events.settings.cpu(), saved["events.settings"]), "the loaded block is the harder one"
        resumed.learn(B * T, reset_num_timesteps=False)
        end = snapshot(resumed)
        fresh.events.set_push(steps=(1, 3))  # (merges with the block as loaded, not with the constructor's settings)
        assert fresh.events.push_norm == (5.0, 25.0) and round(fresh.events.push_prob * 2 ** 24) == round(0.6 * 2 ** 24)
    for k in whole[0]:
        assert same(whole[0][k], end[0][k]), k
    assert same(whole[1][1:], end[1])


def test_an_eval_callback_at_the_top_level_leaves_training_alone():
    from upkie_amd.evaluation import EvalCallback
    from upkie_amd.events import EpisodeEvents, PushLevels

    def learn(with_callback):
        env, policy, model = _make(graph=True)
        with env, pendulum(32, 6, seed=9) as eval_env:
            callback = None
            if with_callback:
                top = EpisodeEvents(eval_env, push_prob=0.5, push_norm=(5.0, 20.0), push_steps=(1, 2), curriculum=PushLevels(3, start=3, up=0, down=0))
                callback = EvalCallback(eval_env, n_eval_episodes=48, eval_freq=T, reward_fn=pitch_reward, seed=9, events=top, chunk=4)
            model.learn(2 * B * T, callback=callback)
            result = snapshot(model)
            if with_callback:
                assert int(top.pushes.sum()) > 0 and bool((top.level == 3).all()) and bool((top.difficulty == 1.0).all())
                assert len(callback.evaluations["timesteps"]) == 2 and all("eval/mean_reward" in r for r in model.records)
            return result

    plain, evald = learn(False), learn(True)
    for k in plain[0]:
        assert same(plain[0][k], evald[0][k]), k
    strip = lambda records: [{k: v for k, v in r.items() if not k.startswith("eval/")} for r in records]  # noqa: E731
    assert same(strip(plain[1]), strip(evald[1]))


def test_the_push_curriculum_example_runs():
    env = dict(os.environ, EXAMPLE_STEPS="16", EXAMPLE_ENVS="64")
    result = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_learn_push_curriculum.py")], capture_output=True, text=True,
                            timeout=600, env=env, cwd=os.path.join(ROOT, "examples"))
    assert result.returncode == 0, result.stderr[-3000:]
    lines = [ln for ln in result.stdout.splitlines() if ln.startswith("iteration")]
    assert len(lines) == 4 and all("envs per level [" in ln for ln in lines), result.stdout
    records = [ln for ln in result.stdout.splitlines() if ln.startswith("record")]
    assert len(records) == 4 and all("rollout/push_level_mean" in ln and "rollout/push_prob" in ln for ln in records), result.stdout
    assert "eval/mean_reward" in result.stdout and "every env still at the top: True" in result.stdout
    assert abi.EVENTS_LEVELS_MAX == 255
