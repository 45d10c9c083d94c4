"""What the episode events (`upkie_amd.events.EpisodeEvents`) cost at 4096 envs (`--num-envs N`: at N) on the pendulum
env. Time per env step, device events around whole graph replays of 128 steps, of

  pushes          the events launch alone, pushes only (each free step starts one with probability 1 %, held 10-30
                  steps), on a handle that is never stepped: nobody ends;
  redraw          the events launch with per-episode inertias on the end-of-episode flags of the pendulum workload
                  itself: steps 337-464 of the env below under the untrained policy, recorded once: the falls of that
                  stretch and the time limit of 400 steps, which ends every surviving episode in ONE step (the line
                  carries the fraction of env steps that end an episode, `finish_rate`, and the largest fraction of the
                  envs that end in one step, `finish_peak`);
  rollout         one graphed `Ppo` rollout step (policy, env, reward, episode statistics, normaliser, bootstrap) with
                  events=None -- the step as it was before the stage existed -- and with pushes and per-episode inertias,
                  two `Ppo` objects in ONE process and build whose replays alternate: `us_per_step` without,
                  `us_per_step_events` with, `us_events` the difference;
  records         separately, the same step with inertial records installed (`inertia_variation=` of the env) and no
                  events: what the step kernels' randomised-inertia instantiations cost, which is theirs and not the
                  stage's, and which `rollout`'s difference contains;
  records_force   the same again with a force buffer of zeros installed on the torso as well
                  (`sim.set_external_force`) and still no events: the instantiations that also read a force. What
                  `rollout` adds beyond this one is the stage's launch and what pushed robots do to the workload.

Each measurement is a child process; the parent interleaves the variants over `--rounds` rounds and prints, per variant,
one JSON line with the median and the spread (min, max) over the rounds. `--variant NAME` runs one measurement in this
process (the program to put behind ``rocprofv3 --kernel-trace --stats --`` for the kernel time of `pushes` / `redraw`).

usage: python tools/bench_episode_events.py [--rounds 5] [--replays 200] [--variant NAME] [--num-envs 4096] [--out profiles/episode_events_bench.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_ENVS, T, LIMIT = 4096, 128, 400
VARIANTS = ("pushes", "redraw", "rollout", "records", "records_force")
LEAD_IN = 336  # env steps before the recorded stretch of `redraw`: the time limit falls inside it
PUSHES = dict(push_prob=0.01, push_norm=(5.0, 20.0), push_steps=(10, 30))


def _time_replays(replay, replays):
    import torch

    for _ in range(3):
        replay()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(replays):
        replay()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / (replays * T)


def _reward(obs, info):
    import torch

    return torch.abs(obs[:, 0]).neg_().add_(1.0)


def _setup(n, **env_kw):
    import torch
    import torch.nn as nn

    import upkie_amd.envs as envs
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    env = envs.make("Upkie-HIP-Pendulum-Vec", num_envs=n, frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=LIMIT,
                    **env_kw)
    dev = env.device
    tower = lambda: nn.Sequential(nn.Linear(4, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)  # noqa: E731
    policy = MlpActorCritic.from_modules(tower(), tower(), nn.Parameter(torch.zeros(1, device=dev)), action_low=[-1.0], action_high=[1.0])
    return env, policy


def _launch_alone(variant, replays, n):
    import torch

    from upkie_amd import abi
    from upkie_amd.events import EpisodeEvents
    from upkie_amd.graphs import GraphedLoop
    from upkie_amd.model.model import Model
    from upkie_amd.sim import BatchedSim

    dev = "cuda:0"
    terminated = torch.zeros(T, n, dtype=torch.bool, device=dev)
    truncated = torch.zeros(T, n, dtype=torch.bool, device=dev)
    extra = {}
    if variant == "redraw":  # the workload's own flags
        env, policy = _setup(n)
        with env:
            action = torch.empty(n, 1, device=dev)
            env.reset(seed=0)
            obs = env.observation
            for t in range(LEAD_IN + T):
                policy.mean_action(obs, action)
                obs, _, term, trunc, _ = env.step(action)
                if t >= LEAD_IN:
                    terminated[t - LEAD_IN].copy_(term)
                    truncated[t - LEAD_IN].copy_(trunc)
            torch.cuda.synchronize()
        ended = (terminated | truncated).float()
        extra["finish_rate"], extra["finish_peak"] = round(float(ended.mean()), 6), round(float(ended.mean(dim=1).max()), 6)
    model = Model()
    sim = BatchedSim(abi.default_sim_config(n), model.struct)  # (never stepped)
    stage_env = types.SimpleNamespace(sim=sim, model=model, num_envs=n, device=sim.device)
    events = EpisodeEvents(stage_env, inertia_variation=0.2 if variant == "redraw" else 0.0, **PUSHES)
    slot = {"t": T - 1}  # (the capture's one warm-up step takes the last slot: the captured steps are 0 .. T - 1)

    def body():
        t = slot["t"]
        events.step(terminated[t], truncated[t])
        slot["t"] = (t + 1) % T

    loop = GraphedLoop(body, unroll=T, warmup=1, device=dev)
    us = _time_replays(loop.replay, replays)
    extra["pushes_per_env_step"] = round(float(events.pushes.sum()) / float(int(events.calls[0]) * n), 6)
    return {"us_per_step": round(us, 3), **extra}


def _ppo(n, events_kw=None, with_force=False, **env_kw):
    import torch

    from upkie_amd.events import EpisodeEvents
    from upkie_amd.ppo import Ppo

    env, policy = _setup(n, **env_kw)
    if with_force:
        env.sim.set_external_force(torch.zeros((3, n), dtype=torch.float32, device=env.device))
    events = EpisodeEvents(env, **events_kw) if events_kw else None
    model = Ppo(env, policy, n_steps=T, batch_size=n * T // 4, reward_fn=_reward, events=events)
    model._setup()  # (captures the rollout: T steps per replay)
    return env, model


def _rollout(variant, replays, n):
    if variant in ("records", "records_force"):
        env, model = _ppo(n, inertia_variation=0.2, with_force=variant == "records_force")
        with env:
            return {"us_per_step": round(_time_replays(model._loop.replay, replays), 3)}
    env_a, plain = _ppo(n)
    env_b, pushed = _ppo(n, dict(inertia_variation=0.2, **PUSHES))
    with env_a, env_b:
        chunk = max(1, replays // 8)
        a, b = [], []
        for _ in range(8):  # alternate, so that a drift of the clocks reaches both alike
            a.append(_time_replays(plain._loop.replay, chunk))
            b.append(_time_replays(pushed._loop.replay, chunk))
        ua, ub = statistics.median(a), statistics.median(b)
        return {"us_per_step": round(ua, 3), "us_per_step_events": round(ub, 3), "us_events": round(ub - ua, 3),
                "pushes_per_env_step": round(float(pushed.events.pushes.sum()) / float(int(pushed.events.calls[0]) * n), 6)}


def measure(variant, replays, n):
    line = {"variant": variant, "num_envs": n, "replays": replays}
    line.update(_launch_alone(variant, replays, n) if variant in ("pushes", "redraw") else _rollout(variant, replays, n))
    print(json.dumps(line), flush=True)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--replays", type=int, default=200)
    parser.add_argument("--variant", choices=VARIANTS)
    parser.add_argument("--out", help="append the result lines to this file")
    parser.add_argument("--num-envs", type=int, default=DEFAULT_ENVS)
    args = parser.parse_args()
    if args.variant:
        measure(args.variant, args.replays, args.num_envs)
        return
    samples = {v: [] for v in VARIANTS}
    for _ in range(args.rounds):
        for variant in VARIANTS:
            cmd = [sys.executable, os.path.abspath(__file__), "--variant", variant, "--replays", str(args.replays), "--num-envs", str(args.num_envs)]
            result = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if result.returncode != 0:
                sys.exit(f"{variant} failed ({result.returncode}):\n{result.stderr[-2000:]}")
            samples[variant].append(json.loads(result.stdout.strip().splitlines()[-1]))
    lines = []
    for variant, runs in samples.items():
        line = {"variant": variant, "rounds": args.rounds, "replays": args.replays, "num_envs": args.num_envs}
        for key in runs[0]:
            if key.startswith("us_"):
                values = [r[key] for r in runs]
                line.update({f"{key}_median": round(statistics.median(values), 3), f"{key}_min": min(values), f"{key}_max": max(values)})
            elif key not in line:
                line[key] = runs[-1][key]
        lines.append(line)
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
