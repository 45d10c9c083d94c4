"""The task targets on the MI355X: the kernel against the fp64 twin (tests/task_targets_reference.py) call by call at every
size and row width, reset and sharding device against device, a captured loop that follows `set_ranges`, the curriculum
launch against its twin over one block and several, and `Ppo` with targets: graphed against eager, save / load, the rows
and the rewards it stores, an `EvalCallback` that leaves training alone, the refusals, the example."""

import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import task_targets_reference as R
from tests.training_rig import bits, read_state, same, snapshot, tower, warm_up_as_the_capture_does
from upkie_amd import abi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stage(num_envs, offset, D, G=None, seed=R.GPU_SEED, **settings):
    """A simulation handle that is never stepped, and the stage on it."""
    from upkie_amd.model.default_model import default_model
    from upkie_amd.sim import BatchedSim
    from upkie_amd.targets import TaskTargets

    cfg = abi.default_sim_config(num_envs, seed=seed)
    cfg.env_id_offset = offset
    sim = BatchedSim(cfg, default_model())
    env = types.SimpleNamespace(sim=sim, num_envs=num_envs, device=sim.device)
    settings = settings or R.gpu_settings(G)
    names = tuple(f"target{g}" for g in range(len(settings["ranges"])))
    return sim, TaskTargets(env, obs_dim=D, names=names, **settings)


def _check_targets(got, want, limits, where):
    """Drawn values within one float32 ulp of max(|low|, |high|) of the twin (the device's one fma rounding is half of
    one; the fp64 twin's own error is negligible beside it); every +0.0 of the twin is +0.0, bit for bit. Returns the worst
    error in ulps."""
    worst = 0.0
    zero = want == 0.0
    assert np.all(bits(got.astype(np.float32))[zero] == 0), f"{where}: a zero target is +0.0 in every bit"
    for g in range(got.shape[0]):
        ulp = float(np.spacing(np.float32(np.abs(limits[g]).max())))
        err = np.abs(got[g].astype(np.float64) - want[g]).max() / ulp
        assert err <= 1.0, (where, g, err)
        worst = max(worst, float(err))
    return worst


@pytest.mark.parametrize("D,G", R.GPU_WIDTHS)
@pytest.mark.parametrize("num_envs,offset", R.GPU_SIZES)
def test_the_kernel_is_the_twin_after_every_call(num_envs, offset, D, G):
    sim, targets = _stage(num_envs, offset, D, G)
    twin = R.Twin(num_envs, D, seed=R.GPU_SEED, env_id_offset=offset, **R.gpu_settings(G))
    limits = twin.limits.astype(np.float64)
    term, trunc = R.gpu_flags(num_envs, offset)
    obs0, nxt, fin = R.gpu_observations(num_envs, D)
    dev = sim.device
    d_term, d_trunc, d_nxt, d_fin = (torch.from_numpy(a).to(dev) for a in (term, trunc, nxt, fin))
    targets.reset(torch.from_numpy(obs0).to(dev))
    twin.reset(obs0)
    prev = read_state(targets)
    assert np.all(prev["calls"] == 1) and np.array_equal(prev["remaining"], twin.remaining) and not prev["final_observation"].any()
    worst = _check_targets(prev["target"], twin.target, limits, "reset")
    assert np.array_equal(bits(prev["observation"][:, :D]), bits(obs0)) and np.array_equal(bits(prev["observation"][:, D:]), bits(prev["target"].T))
    draws = 0
    for t in range(R.GPU_CALLS):
        targets.step(d_nxt[t], d_term[t], d_trunc[t], final_obs=d_fin[t])
        happened = twin.step(nxt[t], term[t], trunc[t], fin[t])
        got = read_state(targets)
        assert np.array_equal(got["calls"].view(np.uint32), twin.calls), t
        assert np.array_equal(got["remaining"], twin.remaining), t
        worst = max(worst, _check_targets(got["target"], twin.target, limits, f"call {t}"))
        held = happened["held"]
        assert np.array_equal(bits(got["target"][:, held]), bits(prev["target"][:, held])), "a held target is not written"
        draws += int(happened["drawn"].sum())
        # the D observation words of both rows: copies, bit for bit
        done = happened["done"]
        assert np.array_equal(bits(got["observation"][:, :D]), bits(nxt[t])), t
        assert np.array_equal(bits(got["final_observation"][:, :D]), bits(np.where(done[:, None], fin[t], nxt[t]))), t
        # the G target words of both rows: the device's own target after and before the call, bit for bit
        assert np.array_equal(bits(got["observation"][:, D:]), bits(got["target"].T)), t
        assert np.array_equal(bits(got["final_observation"][:, D:]), bits(prev["target"].T)), t
        prev = got
    print(f"N = {num_envs}, offset {offset}, (D, G) = ({D}, {G}): {draws} draws, worst |target - twin| {worst:.3g} ulp of the range's end (bound 1)")
    # without a final_obs the terminal row's observation words are next_obs everywhere
    targets.step(d_nxt[0], d_term[0], d_trunc[0])
    got = read_state(targets)
    assert np.array_equal(bits(got["final_observation"][:, :D]), bits(nxt[0])) and np.array_equal(bits(got["final_observation"][:, D:]), bits(prev["target"].T))
    sim.close()


def test_reset_with_a_mask_restarts_only_its_envs():
    N, offset, (D, G) = 65, 1000, (6, 5)
    sim, targets = _stage(N, offset, D, G)
    term, trunc = R.gpu_flags(N, offset)
    obs0, nxt, fin = R.gpu_observations(N, D)
    dev = sim.device
    targets.reset(torch.from_numpy(obs0).to(dev))
    first = read_state(targets)
    for t in range(12):
        targets.step(torch.from_numpy(nxt[t]).to(dev), torch.from_numpy(term[t]).to(dev), torch.from_numpy(trunc[t]).to(dev), final_obs=torch.from_numpy(fin[t]).to(dev))
    moved = read_state(targets)
    assert np.all(moved["calls"] == 13) and not np.array_equal(moved["target"], first["target"])
    mask = np.zeros(N, dtype=np.uint8)
    mask[::3] = 1
    targets.reset(torch.from_numpy(fin[0]).to(dev), torch.from_numpy(mask).to(dev))
    got, m = read_state(targets), mask.astype(bool)
    # the masked envs are back at their first draw, on the new observation; the others and every final row are untouched
    assert np.all(got["calls"][m] == 1) and np.array_equal(got["remaining"][m], first["remaining"][m])
    assert np.array_equal(bits(got["target"][:, m]), bits(first["target"][:, m]))
    assert np.array_equal(bits(got["observation"][m, :D]), bits(fin[0][m])) and np.array_equal(bits(got["observation"][m, D:]), bits(first["target"][:, m].T))
    for name in ("calls", "remaining"):
        assert np.array_equal(got[name][~m], moved[name][~m]), name
    assert np.array_equal(bits(got["target"][:, ~m]), bits(moved["target"][:, ~m])) and np.array_equal(bits(got["observation"][~m]), bits(moved["observation"][~m]))
    assert np.array_equal(bits(got["final_observation"]), bits(moved["final_observation"]))
    sim.close()


def test_one_handle_of_64_is_two_of_32_bit_for_bit():
    D, G = 6, 5
    term, trunc = R.gpu_flags(64, 0)
    obs0, nxt, fin = R.gpu_observations(64, D)

    def run(num_envs, offset, lo):
        sim, targets = _stage(num_envs, offset, D, G)
        part = slice(lo, lo + num_envs)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(sim.device)  # noqa: E731
        targets.reset(up(obs0[part]))
        trace = [read_state(targets)]
        for t in range(R.GPU_CALLS):
            targets.step(up(nxt[t][part]), up(term[t][part]), up(trunc[t][part]), final_obs=up(fin[t][part]))
            trace.append(read_state(targets))
        sim.close()
        return trace

    whole = run(64, 0, 0)
    for lo in (0, 32):
        for a, b in zip(whole, run(32, lo, lo)):
            for name in a:
                if name == "limits":
                    continue
                mine = a[name][:, lo:lo + 32] if name == "target" else a[name][lo:lo + 32]
                assert np.array_equal(bits(mine), bits(b[name])), name


def test_a_captured_loop_follows_set_ranges_and_equals_eager():
    from upkie_amd.graphs import GraphedLoop

    N, D, G = 257, 6, 2
    settings = dict(ranges=[(-0.5, 0.5), (-0.25, 0.25)], resample_steps=(1, 2), stand_prob=0.0)
    obs = torch.from_numpy(R.gpu_observations(N, D)[0]).cuda()

    def run(graphed):
        sim, targets = _stage(N, 1000, D, **settings)
        targets.reset(obs)
        body = lambda: targets.step(obs, None, None)  # noqa: E731
        if graphed:
            loop = GraphedLoop(body, unroll=4, warmup=1, device=sim.device)
        else:
            body()  # (the capture's warm-up step)
            loop = types.SimpleNamespace(replay=lambda: [body() for _ in range(4)])
        loop.replay()
        before = read_state(targets)
        targets.set_ranges([(2.0, 3.0), (-7.0, -6.0)])
        loop.replay()  # (no re-capture)
        after = read_state(targets)
        sim.close()
        return before, after

    (g_before, g_after), (e_before, e_after) = run(True), run(False)
    for a, b in ((g_before, e_before), (g_after, e_after)):
        for name in a:
            assert np.array_equal(bits(a[name]), bits(b[name])), name
    assert np.all(g_before["calls"] == 6) and np.all(g_after["calls"] == 10)
    assert np.all(np.abs(g_before["target"][0]) <= 0.5) and np.all(np.abs(g_before["target"][1]) <= 0.25)
    # holds are 1-2 steps and four steps went by: every env has drawn from the new ranges
    assert np.all((g_after["target"][0] >= 2.0) & (g_after["target"][0] <= 3.0)) and np.all((g_after["target"][1] >= -7.0) & (g_after["target"][1] <= -6.0))
    assert np.array_equal(g_after["limits"], np.array([[2.0, 3.0], [-7.0, -6.0]], dtype=np.float32))


@pytest.mark.parametrize("num_envs", R.CURRICULUM_SIZES)
def test_the_curriculum_launch_is_its_twin(num_envs):
    from upkie_amd.targets import TargetCurriculum

    S = R.CURRICULUM_SETTINGS
    curriculum = TargetCurriculum("track", S["threshold"], S["step"], S["limit"])
    sim, targets = _stage(num_envs, 0, 6, ranges=S["ranges"], resample_steps=(1, 1), curriculum=curriculum)
    score, finished = R.curriculum_inputs(num_envs)
    limits, seen = np.asarray(S["ranges"], dtype=np.float32), np.zeros(num_envs, dtype=np.int32)
    moved = []
    for k in range(6):
        targets.curriculum_step(torch.from_numpy(score[k]).cuda(), torch.from_numpy(finished[k]).cuda())
        moved.append(R.curriculum_step(limits, seen, score[k], finished[k], S["threshold"], S["step"], S["limit"]))
        got = read_state(targets)
        assert np.array_equal(bits(got["limits"]), bits(limits)), (k, got["limits"], limits)
        assert np.array_equal(got["seen"], seen), k
    assert moved == [True, False, True, True, False, False]
    assert not targets._workspace[:8].any(), "the ticket is back to zero for the next launch"
    sim.close()


# ---------------------------------------------------------------- Ppo and the evaluator
B, T, D, G = 64, 8, 6, 2
DT = 1.0 / 200.0


def _gyropod(num_envs, limit, seed=3):
    import upkie_amd.envs as envs
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    init = RobotState(randomization=RobotStateRandomization(pitch=0.3))
    return envs.make("Upkie-HIP-Gyropod-Vec", num_envs=num_envs, frequency=200.0, init_state=init, autoreset_mode="same_step",
                     max_episode_steps=limit, seed=seed)


def _terms():
    from upkie_amd.rewards import Term, obs, one, terminated

    return {"alive": Term(0.5, taps=[one()]), "track": Term(1.0, "exp_square", 0.5, [obs(3), obs(D + 0, -1.0)]),
            "track_yaw": Term(0.5, "exp_square", 0.5, [obs(5), obs(D + 1, -1.0)]), "fall": Term(-2.0, taps=[terminated()])}


def _targets(env, curriculum=True):
    from upkie_amd.targets import TargetCurriculum, TaskTargets

    # (an episode of at most 5 steps sums to at most 5 on "track": a threshold the finished episodes pass in some iterations)
    plan = TargetCurriculum("track", 2.0, step=[0.125, 0.0625], limit=[(-1.0, 1.0), (-0.5, 0.5)]) if curriculum else None
    return TaskTargets(env, ranges=[(-0.5, 0.5), (-0.25, 0.25)], resample_steps=(2, 4), stand_prob=0.2, deadband=[0.05, 0.0], curriculum=plan)


def _make(with_targets=True, curriculum=True, **kw):
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.ppo import Ppo
    from upkie_amd.rewards import RewardTerms

    torch.manual_seed(0)
    env = _gyropod(B, 5, seed=0)
    dev = env.device
    width = D + G if with_targets else D
    policy = MlpActorCritic.from_modules(tower(width, 2).to(dev), tower(width, 1).to(dev), nn.Parameter(torch.zeros(2, device=dev)),
                                         action_low=[-1.0, -1.0], action_high=[1.0, 1.0], seed=0)
    targets = _targets(env, curriculum) if with_targets else None
    reward = RewardTerms(B, D + G, 2, dt=DT, terms=_terms(), device=dev) if with_targets else None
    args = dict(n_steps=T, n_epochs=2, batch_size=B * T // 2, seed=0, reward=reward, targets=targets)
    args.update(kw)
    return env, policy, Ppo(env, policy, **args)


TARGET_KEYS = ("targets.calls", "targets.remaining", "targets.target", "targets.limits", "targets.observation", "targets.final_observation",
               "targets.seen")
ITERATIONS = 3


def test_ppo_with_targets_graphed_equals_not_graphed():
    env, policy, model = _make(graph=True)
    with env:
        model.learn(ITERATIONS * B * T)
        graphed = snapshot(model)
    env, policy, model = _make(graph=False)
    with env:
        warm_up_as_the_capture_does(model)
        model.learn(ITERATIONS * B * T)
        eager = snapshot(model)
    assert all(k in graphed[0] for k in TARGET_KEYS + ("packed", "m", "v", "reward.term_last"))
    for k in graphed[0]:
        assert same(graphed[0][k], eager[0][k]), k
    assert same(graphed[1], eager[1]) and len(graphed[1]) == ITERATIONS
    for record in graphed[1]:
        assert "train/loss" in record and "rollout/ep_rew_track_mean" in record
        for name in ("ground_velocity", "yaw_velocity"):
            assert record[f"rollout/target_{name}_low"] <= record[f"rollout/target_{name}_high"]
    # the warm-up step, then T per iteration, after the reset's call 0
    assert int(graphed[0]["targets.calls"][0]) == ITERATIONS * T + 2
    # the curriculum moved the ranges during the run, inside its limits, and the records show it
    limits = graphed[0]["targets.limits"].cpu().numpy()
    assert limits[0, 1] > 0.5 and limits[0, 1] <= 1.0 and limits[1, 1] > 0.25 and limits[1, 1] <= 0.5 and np.array_equal(limits[:, 0], -limits[:, 1])
    assert graphed[1][-1]["rollout/target_ground_velocity_high"] == float(limits[0, 1])
    # and the targets change the run: a fixed range ends elsewhere
    env, policy, model = _make(curriculum=False, graph=True)
    with env:
        model.learn(ITERATIONS * B * T)
        fixed = snapshot(model)
    assert "targets.seen" not in fixed[0] and not torch.equal(fixed[0]["packed"], graphed[0]["packed"])
    assert fixed[0]["targets.limits"].cpu().tolist() == [[-0.5, 0.5], [-0.25, 0.25]]


def test_ppo_with_targets_resumes_bit_for_bit(tmp_path):
    from upkie_amd.ppo import Ppo

    path = str(tmp_path / "ppo.pt")
    env, policy, model = _make(graph=True)
    with env:
        model.learn(ITERATIONS * B * T)
        whole = snapshot(model)
    env, policy, model = _make(graph=True)
    with env:
        model.learn(ITERATIONS * B * T, callback=lambda m, rec: m.iterations < 2)
        assert model.iterations == 2
        model.save(path)
    env, policy, fresh = _make(graph=True)
    with env:
        resumed = Ppo.load(path, env, policy, n_steps=T, n_epochs=2, batch_size=B * T // 2, seed=0, reward=fresh.reward, targets=fresh.targets)
        resumed.learn(B * T, reset_num_timesteps=False)
        end = snapshot(resumed)
    for k in whole[0]:
        assert same(whole[0][k], end[0][k]), k
    assert same(whole[1][2:], end[1])
    # a file written without targets does not load into a run with them
    env, policy, model = _make(with_targets=False, graph=False)
    with env:
        model.learn(B * T)
        model.save(path)
    env, policy, model = _make(graph=False)
    with env:
        with pytest.raises(ValueError, match=r"the file has no (reward|targets)\."):
            Ppo.load(path, env, policy, n_steps=T, n_epochs=2, batch_size=B * T // 2, seed=0, graph=False, reward=model.reward, targets=model.targets)


def test_the_buffer_holds_the_targets_in_force_and_the_rewards_are_the_reward_twins():
    from tests import reward_terms_reference as W

    env, policy, model = _make(graph=False, normalize=False, bootstrap_time_limits=False)
    with env:
        model._setup()
        targets, agent, rows = model.targets, model._agent, []
        apply = agent.apply

        def recording_apply(action):
            in_force = targets.target.clone()
            out = apply(action)
            rows.append({"in_force": in_force, "action": action.clone(), "final": targets.final_observation.clone(), "terminated": out[2].clone(),
                         "truncated": out[3].clone()})
            return out

        agent.apply = recording_apply
        model.collect_rollouts()
        torch.cuda.synchronize()
        buf = model.buffer
        twin = W.Twin(B, D + G, 2, DT, _terms())
        ended = changed = 0
        for t in range(T):
            row = rows[t]
            # the last G columns of the stored observation are the targets the policy was given at step t
            assert torch.equal(buf.observations[t][:, D:], row["in_force"].T), t
            # ... and the terminal row of step t carries the same ones, whatever was drawn since
            assert torch.equal(row["final"][:, D:], row["in_force"].T), t
            after = targets.target if t == T - 1 else rows[t + 1]["in_force"]
            changed += int((after != row["in_force"]).any(dim=0).sum())
            term, trunc = row["terminated"].cpu().numpy(), row["truncated"].cpu().numpy()
            reward, v, bound = twin.step(row["final"].cpu().numpy(), row["action"].cpu().numpy(), term, trunc, final_obs=None)
            err = np.abs(buf.rewards[t].cpu().numpy().astype(np.float64) - reward)
            allowed = W.Twin.reward_bound(v, bound)
            assert np.all(err <= allowed), (t, float((err / allowed).max()))
            ended += int((term | trunc).sum())
        # (5-step episodes in an 8-step rollout: every env ends one at least; a hold is 2-4 steps: every env draws twice at least)
        assert ended >= B and changed > B, "episodes ended and targets were drawn again during the rollout"


def test_an_eval_callback_with_targets_of_its_own_leaves_training_alone():
    from upkie_amd.evaluation import EvalCallback, evaluate_policy
    from upkie_amd.rewards import RewardTerms
    from upkie_amd.targets import TaskTargets

    def learn(with_callback):
        env, policy, model = _make(graph=True)
        with env, _gyropod(32, 6, seed=9) as eval_env:
            callback = None
            if with_callback:
                eval_targets = TaskTargets(eval_env, ranges=[(-1.0, 1.0), (-0.5, 0.5)], resample_steps=(2, 4))
                eval_reward = RewardTerms(32, D + G, 2, dt=DT, terms=_terms(), device=eval_env.device)
                callback = EvalCallback(eval_env, n_eval_episodes=48, eval_freq=T, reward=eval_reward, seed=9, targets=eval_targets, chunk=4)
            model.learn(2 * B * T, callback=callback)
            result = snapshot(model)
            if with_callback:
                assert int(eval_targets.calls.min()) > 1 and float(eval_targets.target.abs().max()) > 0.5, "the evaluation env draws from its own ranges"
                assert len(callback.evaluations["timesteps"]) == 2 and all("eval/mean_reward" in r for r in model.records)
                runs = [evaluate_policy(policy, eval_env, n_eval_episodes=48, reward=eval_reward, seed=9, targets=eval_targets, chunk=4, graph=g,
                                        return_episode_rewards=True) for g in (True, False)]
                assert runs[0] == runs[1]
            return result

    plain, evald = learn(False), learn(True)
    for k in plain[0]:
        assert same(plain[0][k], evald[0][k]), k
    strip = lambda records: [{k: v for k, v in r.items() if not k.startswith("eval/")} for r in records]  # noqa: E731
    assert same(strip(plain[1]), strip(evald[1]))


def test_refusals_on_the_device():
    from upkie_amd.exceptions import UpkieRuntimeError
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.ppo import Ppo
    from upkie_amd.rewards import RewardTerms, Term, one

    with _gyropod(4, 5) as env:
        dev = env.device
        targets = _targets(env)
        assert targets.obs_dim == D and targets.dim == D + G and set(targets.state_tensors()) == {k.split(".")[1] for k in TARGET_KEYS}
        wide = MlpActorCritic.from_modules(tower(D + G, 2).to(dev), tower(D + G, 1).to(dev), nn.Parameter(torch.zeros(2, device=dev)),
                                           action_low=[-1.0, -1.0], action_high=[1.0, 1.0], seed=0)
        other = RewardTerms(4, D + G, 2, dt=DT, terms={"alive": Term(1.0, taps=[one()])}, device=dev)
        with pytest.raises(ValueError, match="the curriculum reads the reward term 'track'"):
            Ppo(env, wide, reward=other, targets=targets)
        reward = RewardTerms(4, D + G, 2, dt=DT, terms=_terms(), device=dev)
        with pytest.raises(ValueError, match="TargetCurriculum with a process_group"):
            Ppo(env, wide, reward=reward, targets=targets, process_group=object())
        narrow = MlpActorCritic.from_modules(tower(D, 2).to(dev), tower(D, 1).to(dev), nn.Parameter(torch.zeros(2, device=dev)),
                                             action_low=[-1.0, -1.0], action_high=[1.0, 1.0], seed=0)
        with pytest.raises(ValueError, match=f"the policy reads {D} raw observation words, the env's {D} and the {G} targets make {D + G}"):
            Ppo(env, narrow, targets=_targets(env, curriculum=False))
        with pytest.raises(UpkieRuntimeError, match="device tensor"):
            targets.step(torch.zeros(4, D), None, None)
        with pytest.raises(ValueError, match="next_obs"):
            targets.step(torch.zeros(4, D + 1, device=dev), None, None)
        with pytest.raises(UpkieRuntimeError, match="no curriculum"):
            _targets(env, curriculum=False).curriculum_step(reward.term_last[1], reward.finished)
        with pytest.raises(ValueError, match="low <= high"):
            targets.set_ranges([(1.0, -1.0), (0.0, 0.0)])


def test_the_targets_example_runs():
    env = dict(os.environ, EXAMPLE_STEPS="16", EXAMPLE_ENVS="64", EXAMPLE_ITERATIONS="2")
    result = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_learn_targets.py")], capture_output=True, text=True, timeout=600, env=env,
                            cwd=os.path.join(ROOT, "examples"))
    assert result.returncode == 0, result.stderr[-3000:]
    lines = [ln for ln in result.stdout.splitlines() if ln.startswith("iteration")]
    assert len(lines) == 2 and all("train/loss" in ln and "rollout/target_ground_velocity_high" in ln for ln in lines), result.stdout
    assert "eval/mean_reward" in lines[1] and "training ranges:" in result.stdout and "evaluated at the final ranges" in result.stdout
