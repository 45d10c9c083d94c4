"""The episode events on the MI355X: the kernel against the fp64 twin (tests/episode_events_reference.py) call by call on
synthetic end-of-episode flags, reset and sharding device against device, the step kernels reading what the stage wrote,
and `Ppo` / the evaluator with events: graphed against eager, save / load, an `EvalCallback` that leaves training alone,
the example."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import episode_events_reference as R
from tests.training_rig import (bits, check_event_records, events_stage, pendulum, pitch_reward, read_state, same, snapshot, tower,
                                warm_up_as_the_capture_does)
from upkie_amd import abi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_NORM = R.GPU_SETTINGS["push_norm"][1]


@pytest.fixture(scope="module")
def model():
    from upkie_amd.model.model import Model

    return Model()  # URDF-derived: 13 links behind 7 bodies


def _stage(model, num_envs, offset, seed=R.GPU_SEED, **settings):
    return events_stage(model, num_envs, offset, seed, **(settings or R.GPU_SETTINGS))


@pytest.mark.parametrize("num_envs,offset", R.GPU_SIZES)
def test_the_kernel_is_the_twin_after_every_call(model, num_envs, offset):
    sim, events = _stage(model, num_envs, offset)
    twin = R.Twin(model.struct, num_envs, seed=R.GPU_SEED, env_id_offset=offset, **R.GPU_SETTINGS)
    assert events.threshold == twin.threshold == 2 ** 22
    assert sim.ext_force.data_ptr() == events.force.data_ptr() and sim.body_inertials.data_ptr() == events.body_inertials.data_ptr()
    term, trunc = R.gpu_flags(num_envs, offset)
    d_term, d_trunc = torch.from_numpy(term).to(sim.device), torch.from_numpy(trunc).to(sim.device)
    every = np.arange(num_envs)
    prev = read_state(events)
    check_event_records(prev, twin.snapshot(), every)  # construction: episode 0
    worst_force, worst_record, starts = 0.0, 0.0, 0
    for t in range(R.GPU_CALLS):
        events.step(d_term[t], d_trunc[t])
        happened = twin.step(term[t], trunc[t])
        got, want = read_state(events), twin.snapshot()
        for name in ("calls", "remaining", "pushes", "episodes"):
            assert np.array_equal(bits(got[name]), bits(want[name].astype(np.uint32) if name != "remaining" else want[name])), (name, t)
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
            ref = want["body_inertials"][:, done]
            worst_record = max(worst_record, float((np.abs(got["body_inertials"][:, done] - ref) / (3e-5 * np.abs(ref) + 1e-9)).max()))
        for name in ("body_inertials", "link_scale"):
            assert np.array_equal(bits(got[name][:, ~done]), bits(prev[name][:, ~done])), f"{name} of envs that did not end is not written"
        prev = got
    print(f"N = {num_envs}, offset {offset}: {starts} starts, worst |force - twin| {worst_force:.3g} N (bound {2e-6 * MAX_NORM:.3g}), "
          f"worst record error / bound {worst_record:.3g}")
    assert worst_force < 2e-6 * MAX_NORM
    sim.close()


def test_reset_gives_randomize_inertias_and_a_mask_restarts_only_its_envs(model):
    from upkie_amd.sim import BatchedSim

    N, offset = 65, 1000
    sim, events = _stage(model, N, offset)
    cfg = abi.default_sim_config(N, seed=R.GPU_SEED)
    cfg.env_id_offset = offset
    other = BatchedSim(cfg, model.struct)
    want = {"body_inertials": other.randomize_inertias(0.3).cpu().numpy().astype(np.float64), "link_scale": other.link_scale.cpu().numpy()}
    term, trunc = R.gpu_flags(N, offset)
    d_term, d_trunc = torch.from_numpy(term).to(sim.device), torch.from_numpy(trunc).to(sim.device)
    check_event_records(read_state(events), want, np.arange(N))
    for t in range(12):
        events.step(d_term[t], d_trunc[t])
    moved = read_state(events)
    assert moved["episodes"].max() >= 1 and moved["pushes"].max() >= 1 and np.all(moved["calls"] == 12)
    mask = np.zeros(N, dtype=np.uint8)
    mask[::3] = 1
    events.reset(torch.from_numpy(mask).to(sim.device))
    got, m = read_state(events), mask.astype(bool)
    for name in ("calls", "remaining", "pushes", "episodes"):
        assert np.all(got[name][m] == 0) and np.array_equal(got[name][~m], moved[name][~m]), name
    assert np.all(bits(got["force"][0][:, m]) == 0)
    for name in ("force", "body_inertials", "link_scale"):
        assert np.array_equal(bits(got[name][..., ~m]), bits(moved[name][..., ~m])), name
    check_event_records(got, want, np.flatnonzero(m))
    events.reset()
    got = read_state(events)
    assert all(not got[name].any() for name in ("calls", "remaining", "pushes", "episodes", "force"))
    check_event_records(got, want, np.arange(N))
    # the same bits as the handle's own draw: one arithmetic, one key
    assert np.array_equal(bits(got["body_inertials"]), bits(other.body_inertials.cpu().numpy()))
    sim.close()
    other.close()


def test_one_handle_of_64_is_two_of_32_bit_for_bit(model):
    term, trunc = R.gpu_flags(64, 0)

    def run(num_envs, offset, lo):
        sim, events = _stage(model, num_envs, offset)
        d_term = torch.from_numpy(np.ascontiguousarray(term[:, lo:lo + num_envs])).to(sim.device)
        d_trunc = torch.from_numpy(np.ascontiguousarray(trunc[:, lo:lo + num_envs])).to(sim.device)
        trace = []
        for t in range(R.GPU_CALLS):
            events.step(d_term[t], d_trunc[t])
            trace.append(read_state(events))
        sim.close()
        return trace

    whole = run(64, 0, 0)
    for lo in (0, 32):
        for a, b in zip(whole, run(32, lo, lo)):
            for name in a:
                assert np.array_equal(bits(a[name][..., lo:lo + 32]), bits(b[name])), name


# ---------------------------------------------------------------- the step kernels read what the stage wrote
def test_the_sim_steps_under_the_force_and_the_records_the_stage_wrote(model):
    from upkie_amd.events import EpisodeEvents

    N = 65
    rng = np.random.default_rng(8)
    with pendulum(N, 7, seed=3, model=model) as a, pendulum(N, 7, seed=3, model=model) as b, pendulum(N, 7, seed=3, model=model) as plain:
        events = EpisodeEvents(a, push_prob=0.5, push_norm=(5.0, 20.0), push_steps=(1, 3), inertia_variation=0.3)
        body, point, _ = model.link_attachment("torso")
        assert body == 0
        force_b = torch.zeros((3, N), dtype=torch.float32, device=b.device)
        records_b = torch.zeros_like(events.body_inertials)
        b.sim.set_external_force(force_b, point=tuple(float(x) for x in point))
        b.sim.set_body_inertials(records_b)
        assert b.sim.ext_force.data_ptr() == force_b.data_ptr() and b.sim.body_inertials.data_ptr() == records_b.data_ptr()
        records_b.copy_(events.body_inertials)  # (episode 0: a reset steps the physics once, with the env's inertials)
        for env in (a, b, plain):
            env.reset(seed=3)
        events.reset()
        records_b.copy_(events.body_inertials)
        ended = 0
        for k in range(30):
            act = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(N, 1)).astype(np.float32)).to(a.device)
            force_b.copy_(events.force[0])
            records_b.copy_(events.body_inertials)
            out_a = a.step(act)
            events.step(out_a[2], out_a[3])
            out_b = b.step(act)
            out_p = plain.step(act)
            torch.cuda.synchronize()
            for x, y, name in zip(out_a[:4], out_b[:4], ("observation", "reward", "terminated", "truncated")):
                assert torch.equal(x, y), (name, k)
            assert torch.equal(a.sim.state, b.sim.state), k
            assert torch.equal(out_a[4]["final_obs"], out_b[4]["final_obs"]), k
            ended += int((out_a[2] | out_a[3]).sum())
        assert ended >= 4 * N and int(events.pushes.sum()) > N and int(events.episodes.sum()) == ended
        # the same actions without the stage end elsewhere (the difference tests/test_parity_gpu.py asks of a randomisation)
        assert float((out_p[0] - out_a[0]).abs().max()) > 1e-3


# ---------------------------------------------------------------- Ppo and the evaluator
B, T = 64, 8
SETTINGS = dict(push_prob=0.1, push_norm=(5.0, 20.0), push_steps=(1, 3), inertia_variation=0.2)


def _make(with_events=True, **kw):
    from upkie_amd.events import EpisodeEvents
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.ppo import Ppo

    torch.manual_seed(0)
    env = pendulum(B, 5, seed=0)
    dev = env.device
    policy = MlpActorCritic.from_modules(tower(4, 1).to(dev), tower(4, 1).to(dev), nn.Parameter(torch.zeros(1, device=dev)), action_low=[-1.0],
                                         action_high=[1.0], seed=0)
    events = EpisodeEvents(env, **SETTINGS) if with_events else None
    model = Ppo(env, policy, n_steps=T, n_epochs=2, batch_size=B * T // 2, seed=0, reward_fn=pitch_reward, events=events, **kw)
    return env, policy, model


EVENT_KEYS = ("events.calls", "events.remaining", "events.pushes", "events.episodes", "events.force", "events.body_inertials", "events.link_scale")


def test_ppo_with_events_graphed_equals_not_graphed():
    env, policy, model = _make(graph=True)
    with env:
        model.learn(2 * B * T)
        graphed = snapshot(model)
    env, policy, model = _make(graph=False)
    with env:
        warm_up_as_the_capture_does(model)
        model.learn(2 * B * T)
        eager = snapshot(model)
    assert all(k in graphed[0] for k in EVENT_KEYS + ("packed", "m", "v"))
    for k in graphed[0]:
        assert same(graphed[0][k], eager[0][k]), k
    assert same(graphed[1], eager[1]) and len(graphed[1]) == 2 and all("train/loss" in r for r in graphed[1])
    assert int(graphed[0]["events.calls"][0]) == 2 * T + 1 and graphed[0]["events.pushes"].sum() > 0 and graphed[0]["events.episodes"].sum() > 0
    # and the events change the run: without them it ends elsewhere
    env, policy, model = _make(with_events=False, graph=True)
    with env:
        model.learn(2 * B * T)
        plain = snapshot(model)
    assert not any(k.startswith("events.") for k in plain[0]) and not torch.equal(plain[0]["packed"], graphed[0]["packed"])


def test_ppo_with_events_resumes_bit_for_bit(tmp_path):
    from upkie_amd.events import EpisodeEvents
    from upkie_amd.ppo import Ppo

    path = str(tmp_path / "ppo.pt")
    env, policy, model = _make(graph=True)
    with env:
        model.learn(2 * B * T)
        whole = snapshot(model)
    env, policy, model = _make(graph=True)
    with env:
        model.learn(2 * B * T, callback=lambda m, rec: m.iterations < 1)
        assert model.iterations == 1
        model.save(path)
    env, policy, fresh = _make(graph=True)
    with env:
        resumed = Ppo.load(path, env, policy, n_steps=T, n_epochs=2, batch_size=B * T // 2, seed=0, reward_fn=pitch_reward, events=fresh.events)
        resumed.learn(B * T, reset_num_timesteps=False)
        end = snapshot(resumed)
    for k in whole[0]:
        assert same(whole[0][k], end[0][k]), k
    assert same(whole[1][1:], end[1])
    # a file written without events loads as before, and not into a run with events
    env, policy, model = _make(with_events=False, graph=False)
    with env:
        model.learn(B * T)
        model.save(path)
    env, policy, model = _make(with_events=False, graph=False)
    with env:
        assert Ppo.load(path, env, policy, n_steps=T, n_epochs=2, batch_size=B * T // 2, seed=0, graph=False, reward_fn=pitch_reward).iterations == 1
        with pytest.raises(ValueError, match="events.calls"):
            Ppo.load(path, env, policy, n_steps=T, n_epochs=2, batch_size=B * T // 2, seed=0, graph=False, reward_fn=pitch_reward,
                     events=EpisodeEvents(env, **SETTINGS))


def test_an_eval_callback_with_events_of_its_own_leaves_training_alone():
    from upkie_amd.evaluation import EvalCallback, evaluate_policy
    from upkie_amd.events import EpisodeEvents

    def learn(with_callback):
        env, policy, model = _make(graph=True)
        with env, pendulum(32, 6, seed=9) as eval_env:
            callback, eval_events = None, None
            if with_callback:
                eval_events = EpisodeEvents(eval_env, push_prob=0.5, push_norm=(5.0, 20.0), push_steps=(1, 2))
                callback = EvalCallback(eval_env, n_eval_episodes=48, eval_freq=T, reward_fn=pitch_reward, seed=9, events=eval_events, chunk=4)
            model.learn(2 * B * T, callback=callback)
            result = snapshot(model)
            if with_callback:
                assert int(eval_events.pushes.sum()) > 0, "the evaluation env is pushed"
                assert len(callback.evaluations["timesteps"]) == 2 and all("eval/mean_reward" in r for r in model.records)
                # graphed and eager evaluations under events give the same episodes
                runs = [evaluate_policy(policy, eval_env, n_eval_episodes=48, reward_fn=pitch_reward, seed=9, events=eval_events, chunk=4, graph=g,
                                        return_episode_rewards=True) for g in (True, False)]
                assert runs[0] == runs[1]
            return result

    plain, evald = learn(False), learn(True)
    for k in plain[0]:
        assert same(plain[0][k], evald[0][k]), k
    strip = lambda records: [{k: v for k, v in r.items() if not k.startswith("eval/")} for r in records]  # noqa: E731
    assert same(strip(plain[1]), strip(evald[1]))


def test_construction_refuses_forces_already_there_and_host_flags(model):
    from upkie_amd.events import EpisodeEvents
    from upkie_amd.exceptions import UpkieRuntimeError

    with pendulum(4, 5, seed=3) as env:
        env.set_external_forces("torso", torch.tensor([1.0, 0.0, 0.0]))
        with pytest.raises(ValueError, match="already carries external forces"):
            EpisodeEvents(env, push_prob=0.5)
        env.set_external_forces("torso", None)
        events = EpisodeEvents(env, push_prob=0.5, push_link="left_wheel_tire")
        assert env.sim.ext_force.data_ptr() == events.force.data_ptr() and env.sim.body_inertials is None
        assert set(events.state_tensors()) == {"calls", "remaining", "pushes", "episodes", "force"}
        with pytest.raises(UpkieRuntimeError, match="device tensor"):
            events.step(torch.zeros(4, dtype=torch.uint8), None)
        with pytest.raises(ValueError, match="terminated"):
            events.step(torch.zeros(5, dtype=torch.uint8, device=env.device), None)
        events.step(None, None)
        torch.cuda.synchronize()
        assert int(events.calls[0]) == 1


def test_the_events_example_runs():
    env = dict(os.environ, EXAMPLE_STEPS="16", EXAMPLE_ENVS="64")
    result = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_learn_events.py")], capture_output=True, text=True, timeout=600, env=env,
                            cwd=os.path.join(ROOT, "examples"))
    assert result.returncode == 0, result.stderr[-3000:]
    lines = [ln for ln in result.stdout.splitlines() if ln.startswith("iteration")]
    assert len(lines) == 3 and all("train/loss" in ln for ln in lines), result.stdout
    assert "evaluate_policy, pushed:" in result.stdout and "evaluate_policy, not pushed:" in result.stdout and "pushes started" in result.stdout
