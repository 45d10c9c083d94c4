"""What the task targets (`upkie_amd.targets.TaskTargets`, `Ppo(targets=...)`) cost at 4096 envs (`--num-envs N`: at N).
Device events around `--iters` back-to-back launches, `--repeats` samples each; one JSON line per variant with the median
and the range (min, max) over the samples; the stage and its yardstick also replayed from a hipGraph of 100 launches
(`us_graphed_*`: the device's time per launch, without the host's launch cost that an eager call from Python mostly is):

  stage_6_2, stage_248_8       the stage's launch at (D, G) = (6, 2) and (248, 8), an episode ending in 0.5 % of the envs
                               and holds of 200-600 steps (the example's);
  privileged_8, privileged_256 `upkie_privileged_observation` moving rows of the same widths (one observation segment of
                               8 and of 256 words): the nearest existing yardstick, from the same run;
  redraw_6_2                   the stage with holds of one step: every env draws at every call (the cost of the draw);
  curriculum, curriculum_262144  the curriculum's launch at N and at 262144 envs, every env newly finished;
  rollout                      one graphed `Ppo` rollout step of examples/ppo_learn_reward_terms.py's configuration
                               (pendulum env, `AgentPipeline` of 8 frames, `RewardTerms`) without and with `targets=`
                               (G = 1: a ground velocity, tracked by one more term), two `Ppo` objects whose replays
                               alternate: `us_per_step`, `us_per_step_targets`, `us_targets` the difference.

`--tree DIR` imports the package from another checkout of the project that has been built (the parent commit, for the
"without" side of `rollout`): a tree without the feature runs that side only.

usage: python tools/bench_task_targets.py [--tree DIR] [--label NAME] [--repeats 5] [--iters 200] [--num-envs 4096]
                                          [--out profiles/task_targets_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _time(fn, iters, repeats):
    """Microseconds per call of `fn`: `repeats` samples of `iters` calls between two device events."""
    import torch

    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        samples.append(start.elapsed_time(end) * 1e3 / iters)
    return samples


def _both(fn, iters, repeats, device):
    """`fn` launched eagerly from Python (mostly the host's launch cost) and replayed from a hipGraph of 100 launches (the
    device's own time per launch: `us_graphed_*`)."""
    from upkie_amd.graphs import GraphedLoop

    eager = _time(fn, iters, repeats)
    loop = GraphedLoop(fn, unroll=100, warmup=1, device=device)
    graphed = [us / 100 for us in _time(loop.replay, max(1, iters // 20), repeats)]
    return dict(_figures(eager), **_figures(graphed, "us_graphed"))


def _figures(samples, key="us"):
    return {f"{key}_median": round(statistics.median(samples), 3), f"{key}_min": round(min(samples), 3), f"{key}_max": round(max(samples), 3)}


def _handle(n):
    """An env that is never stepped: a simulation handle (the seed and the global ids), the size, the device."""
    from upkie_amd import abi
    from upkie_amd.model.default_model import default_model
    from upkie_amd.sim import BatchedSim

    sim = BatchedSim(abi.default_sim_config(n, seed=0), default_model())
    return types.SimpleNamespace(sim=sim, num_envs=n, device=sim.device)


def stage_launch(n, d, g, iters, repeats, resample_steps=(200, 600)):
    import torch

    from upkie_amd.targets import TaskTargets

    env = _handle(n)
    stage = TaskTargets(env, obs_dim=d, names=[f"t{k}" for k in range(g)], ranges=[(-1.0, 1.0)] * g, resample_steps=resample_steps, stand_prob=0.1)
    obs, final = torch.randn(n, d, device=env.device), torch.randn(n, d, device=env.device)
    done = (torch.rand(n, device=env.device) < 0.005).to(torch.uint8)
    stage.reset(obs)
    out = dict(_both(lambda: stage.step(obs, done, None, final_obs=final), iters, repeats, env.device), row_words=stage.dim)
    env.sim.close()
    return out


def privileged_launch(n, words, iters, repeats):
    import torch

    from upkie_amd.privileged import PrivilegedObservation

    dev = torch.device("cuda:0")
    env = types.SimpleNamespace(num_envs=n, device=dev)
    stage = PrivilegedObservation(env, include=("observation",), obs_dim=words)
    obs, final = torch.randn(n, words, device=dev), torch.randn(n, words, device=dev)
    done = (torch.rand(n, device=dev) < 0.005).to(torch.uint8)
    stage.reset(obs)
    return dict(_both(lambda: stage.step(obs, done, None, final_obs=final), iters, repeats, dev), row_words=stage.dim)


def curriculum_launch(n, iters, repeats):
    import torch

    from upkie_amd.targets import TargetCurriculum, TaskTargets

    env = _handle(n)
    plan = TargetCurriculum("track", 0.5, step=[0.0, 0.0], limit=[(-1.0, 1.0)] * 2)  # (a step of 0: every launch decides, the ranges stay)
    stage = TaskTargets(env, obs_dim=6, resample_steps=(200, 600), curriculum=plan)
    score = torch.rand(n, dtype=torch.float64, device=env.device) + 0.5
    finished = torch.ones(n, dtype=torch.int32, device=env.device)

    def look():  # (every env newly finished at every launch: `seen` is put back by a fill the yardstick below times alone)
        stage.seen.zero_()
        stage.curriculum_step(score, finished)

    both, fill = _time(look, iters, repeats), _time(stage.seen.zero_, iters, repeats)
    out = dict(_figures(both, "us_with_fill"), **_figures(fill, "us_fill"))
    out["us_median"] = round(out["us_with_fill_median"] - out["us_fill_median"], 3)
    env.sim.close()
    return out


def _tower(d_in, d_out, dev):
    import torch.nn as nn

    return nn.Sequential(nn.Linear(d_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, d_out)).to(dev)


def _ppo(n, with_targets):
    """examples/ppo_learn_reward_terms.py's configuration; with targets a commanded ground velocity and its tracking term."""
    import torch
    import torch.nn as nn

    import upkie_amd.envs as envs
    from upkie_amd.pipeline import AgentPipeline
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.ppo import Ppo
    from upkie_amd.rewards import RewardTerms, Term, act_rate, obs, one, terminated
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    env = envs.make("Upkie-HIP-Pendulum-Vec", num_envs=n, frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=400)
    dev, g = env.device, 1 if with_targets else 0
    terms = {"alive": Term(1.0, taps=[one()]), "upright": Term(-1.0, "abs", taps=[obs(0)]), "in_place": Term(-0.25, "abs", taps=[obs(1)]),
             "action_rate": Term(-0.01, "square", taps=[act_rate(0)]), "fall": Term(-10.0, taps=[terminated()])}
    kw = {}
    if with_targets:
        from upkie_amd.targets import TaskTargets

        terms["track"] = Term(1.0, "exp_square", 0.25, [obs(3), obs(4, -1.0)])
        kw["targets"] = TaskTargets(env, names=("ground_velocity",), ranges=[(-0.5, 0.5)], resample_steps=(200, 600), stand_prob=0.1)
    pipe = AgentPipeline(n, 4 + g, [-1.0], [1.0], dt=1.0 / 200.0, stack=8, integrate_action=True, action_noise=[0.02], action_lag=0.05,
                         observation_noise=[0.002, 0.002, 0.01, 0.01] + [0.0] * g, seed=0, device=dev)
    reward = RewardTerms(n, 4 + g, 1, dt=1.0 / 200.0, terms=terms, device=dev)
    width = pipe.stacked_dim
    policy = MlpActorCritic.from_modules(_tower(width, 1, dev), _tower(width, 1, dev), nn.Parameter(torch.zeros(1, device=dev)), action_low=[-2.0],
                                         action_high=[2.0])
    model = Ppo(env, policy, n_steps=128, batch_size=n * 128 // 4, reward=reward, pipeline=pipe, **kw)
    model._setup()  # (captures the rollout: 128 steps per replay)
    return env, model


def rollout(n, iters, repeats, feature):
    env_a, plain = _ppo(n, False)
    replays = max(1, iters // 40)
    if not feature:
        with env_a:
            return _figures([us / 128 for us in _time(plain._loop.replay, replays, repeats)], "us_per_step")
    env_b, goal = _ppo(n, True)
    with env_a, env_b:
        a, b = [], []
        for _ in range(repeats):  # alternate, so that a drift of the clocks reaches both alike
            a += [us / 128 for us in _time(plain._loop.replay, replays, 1)]
            b += [us / 128 for us in _time(goal._loop.replay, replays, 1)]
        out = dict(_figures(a, "us_per_step"), **_figures(b, "us_per_step_targets"))
        out["us_targets"] = round(out["us_per_step_targets_median"] - out["us_per_step_median"], 3)
        return out


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--tree", default=ROOT, help="the checkout whose package is measured (default: this one)")
    parser.add_argument("--label", default="this tree")
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--iters", type=int, default=200)
    parser.add_argument("--num-envs", type=int, default=4096)
    parser.add_argument("--out", help="append the result lines to this file")
    args = parser.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import importlib.util

    feature = importlib.util.find_spec("upkie_amd.targets") is not None
    n, it, rep = args.num_envs, args.iters, args.repeats
    variants = []
    if feature:
        variants += [("stage_6_2", lambda: stage_launch(n, 6, 2, it, rep)), ("privileged_8", lambda: privileged_launch(n, 8, it, rep)),
                     ("stage_248_8", lambda: stage_launch(n, 248, 8, it, rep)), ("privileged_256", lambda: privileged_launch(n, 256, it, rep)),
                     ("redraw_6_2", lambda: stage_launch(n, 6, 2, it, rep, resample_steps=(1, 1))),
                     ("curriculum", lambda: curriculum_launch(n, it, rep)), ("curriculum_262144", lambda: curriculum_launch(262144, it, rep))]
    variants.append(("rollout", lambda: rollout(n, it, rep, feature)))
    lines = []
    for name, run in variants:
        line = {"variant": name, "tree": args.label, "num_envs": n, "repeats": rep, "iters": it}
        line.update(run())
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
