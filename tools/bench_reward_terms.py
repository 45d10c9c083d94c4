"""What the reward terms (`upkie_amd.rewards.RewardTerms`, one launch per step) cost at 4096 envs, D = 4, A = 1, with the
five terms of examples/ppo_learn_reward_terms.py. Time per step, device events around whole graph replays, of

  launch   `RewardTerms.step` alone, 128 steps per replay on fixed inputs;
  terms    the graphed 128-step rollout of examples/ppo_learn_pipeline.py with ``Ppo(reward=RewardTerms(...))``;
  torch    the same rollout with that example's ``reward_fn`` (five torch ops per step; `Ppo`'s ``reward_fn`` path is the
           code of the commit before the reward terms existed).

Each measurement is a child process; the parent interleaves the variants over `--rounds` rounds and prints, per variant,
one JSON line with the median and the spread (min, max) over the rounds, then ``terms - torch``. `--variant NAME` runs
one measurement in this process (the program to put behind ``rocprofv3 --kernel-trace --stats --``).

usage: python tools/bench_reward_terms.py [--rounds 5] [--replays 20] [--variant NAME] [--out profiles/reward_terms_bench.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

N, K, D, A, T = 4096, 8, 4, 1, 128
DT = 1.0 / 200.0
VARIANTS = ("launch", "terms", "torch")


def _terms():
    import importlib

    return importlib.import_module("ppo_learn_reward_terms").terms()


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


def _launch(replays):
    import torch

    from upkie_amd.graphs import GraphedLoop
    from upkie_amd.rewards import RewardTerms

    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    reward = RewardTerms(N, D, A, DT, _terms(), device=dev)
    obs, final = (torch.rand(N, D, device=dev, generator=gen) - 0.5 for _ in range(2))
    action = torch.rand(N, A, device=dev, generator=gen) * 2 - 1
    terminated = torch.rand(N, device=dev, generator=gen) < 0.01
    truncated = torch.rand(N, device=dev, generator=gen) < 0.01
    loop = GraphedLoop(lambda: reward.step(obs, action, terminated, truncated, final_obs=final), unroll=T, warmup=3, device=dev)
    return _time_replays(loop.replay, replays)


def _rollout(variant, replays):
    import torch
    import torch.nn as nn

    import upkie_amd.envs as envs
    from upkie_amd.pipeline import AgentPipeline
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.ppo import Ppo
    from upkie_amd.rewards import RewardTerms
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=N, frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=400) as env:
        dev = env.device
        pipe = AgentPipeline(N, D, [-1.0], [1.0], dt=DT, stack=K, integrate_action=True, action_noise=[0.02], action_lag=0.05,
                             observation_noise=[0.002, 0.002, 0.01, 0.01], seed=0, device=dev)
        words = pipe.stacked_dim
        tower = lambda: nn.Sequential(nn.Linear(words, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)  # noqa: E731
        policy = MlpActorCritic.from_modules(tower(), tower(), nn.Parameter(torch.zeros(1, device=dev)), action_low=[-2.0], action_high=[2.0])
        if variant == "terms":
            kw = {"reward": RewardTerms(N, D, A, DT, _terms(), device=dev)}
        else:  # examples/ppo_learn_pipeline.py's reward
            kw = {"reward_fn": lambda obs, info: torch.abs(obs[:, 1]).mul_(-0.25).sub_(torch.abs(obs[:, 0])).add_(1.0)}
        model = Ppo(env, policy, n_steps=T, batch_size=N * T // 4, pipeline=pipe, **kw)
        model._setup()
        return _time_replays(model._loop.replay, replays)


def measure(variant, replays):
    us = _launch(replays) if variant == "launch" else _rollout(variant, replays)
    print(json.dumps({"variant": variant, "us_per_step": round(us, 3), "num_envs": N, "obs_dim": D, "act_dim": A, "terms": len(_terms()),
                      "n_steps": T, "replays": replays}), flush=True)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--replays", type=int, default=20)
    parser.add_argument("--variant", choices=VARIANTS)
    parser.add_argument("--out", help="append the result lines to this file")
    args = parser.parse_args()
    if args.variant:
        measure(args.variant, args.replays)
        return
    samples = {v: [] for v in VARIANTS}
    for _ in range(args.rounds):
        for variant in VARIANTS:
            cmd = [sys.executable, os.path.abspath(__file__), "--variant", variant, "--replays", str(args.replays)]
            result = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if result.returncode != 0:
                sys.exit(f"{variant} failed ({result.returncode}):\n{result.stderr[-2000:]}")
            samples[variant].append(json.loads(result.stdout.strip().splitlines()[-1])["us_per_step"])
    lines = []
    for variant, values in samples.items():
        lines.append({"variant": variant, "us_per_step_median": round(statistics.median(values), 3), "min": min(values), "max": max(values),
                      "rounds": args.rounds, "replays": args.replays, "num_envs": N, "n_steps": T, "terms": 5})
    lines.append({"difference": "terms - torch", "us_per_step": round(statistics.median(samples["terms"]) - statistics.median(samples["torch"]), 3),
                  "rounds": args.rounds})
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
