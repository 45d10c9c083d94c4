"""What on-device evaluation (`upkie_amd.evaluation`) costs at 4096 envs and 4096 episodes (`--num-envs N`: at N and N)
on the pendulum env with a [64, 64] tanh policy. Time per step, device events around whole graph replays of 128 steps, of

  tally      `EpisodeTally.step` alone on a [128, 4096] stream of flags in which 31 OTHER envs end on every step (a
             random permutation of the envs, 31 at a time, alternately terminated and truncated), so that every step of a
             replay appends 31 records; the tally is reset before every replay, one more launch per 128 steps, and with
             128 x 31 = 3968 < 4096 records the list is never full: no step here writes the summary;
  idle       the same launch when no env under quota ends (every step after the list is full, and a step in which
             nobody ends): nothing to place;
  episodes   `EpisodeStatistics.step` (window 100) on the tally's stream: the yardstick, the same per-env pass and prefix,
             31 episodes into the ring and the ring's means every step;
  step       one graphed evaluation step (policy, env, reward, tally);
  no_tally   the same step without the tally;

and wall time, host clock around a synchronised call, of

  evaluate   a whole `evaluate_policy` of 4096 episodes, graphed, 32 steps per replay (the loop already captured);
  torch      the same evaluation as a Python loop with torch ops and a per-step host gather of the finished envs.

Each measurement is a child process; the parent interleaves the variants over `--rounds` rounds and prints, per variant,
one JSON line with the median and the spread (min, max) over the rounds. `--variant NAME` runs one measurement in this
process (the program to put behind ``rocprofv3 --kernel-trace --stats --`` for the kernel times of `tally` / `idle` /
`episodes`, each in a run of its own).

`--replays` counts graph replays of 128 steps for the per-step variants (400: a quarter of a second of tally launches) and
a tenth as many whole evaluations for `evaluate` / `torch`; every result line records the count it used.

`--num-envs N` takes every measurement at N envs and N episodes instead (262145: 1021 blocks in the bookkeeping kernels).

usage: python tools/bench_evaluation.py [--rounds 5] [--replays 400] [--variant NAME] [--num-envs 4096] [--out profiles/evaluation_bench.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_ENVS, T, LIMIT = 4096, 128, 400  # (N envs and E = N episodes: every measurement takes `n`)
PER_STEP = 31  # envs that end on each step of the tally's stream: T x PER_STEP < E, so the list never fills
VARIANTS = ("tally", "idle", "episodes", "step", "no_tally", "evaluate", "torch")
UNITS = {"evaluate": "ms_per_evaluation", "torch": "ms_per_evaluation"}


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


def _bookkeeping(variant, replays, n):
    N = E = n
    import torch

    from upkie_amd.episodes import EpisodeStatistics
    from upkie_amd.evaluation import EpisodeTally
    from upkie_amd.graphs import GraphedLoop

    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    reward = torch.rand(T, N, device=dev, generator=gen)
    terminated = torch.zeros(T, N, dtype=torch.bool, device=dev)
    truncated = torch.zeros(T, N, dtype=torch.bool, device=dev)
    if variant != "idle":
        order = torch.randperm(N, device=dev, generator=gen)[:T * PER_STEP].reshape(T, PER_STEP)
        steps = torch.arange(T, device=dev)[:, None].expand(T, PER_STEP)
        terminated[steps[:, 0::2], order[:, 0::2]] = True
        truncated[steps[:, 1::2], order[:, 1::2]] = True
        assert int((terminated | truncated).sum(dim=1).min()) == PER_STEP and int((terminated | truncated).sum(dim=0).max()) == 1
    slot = {"t": T - 1}  # (the capture's one warm-up step takes the last slot: the captured steps are 0 .. T - 1)

    def stream(step):
        def body():
            t = slot["t"]
            step(reward[t], terminated[t], truncated[t])
            slot["t"] = (t + 1) % T

        return body

    if variant == "episodes":
        stats = EpisodeStatistics(N, window=100, device=dev)
        loop = GraphedLoop(stream(stats.step), unroll=T, warmup=1, device=dev)
        return _time_replays(loop.replay, replays)
    tally = EpisodeTally(N, E, device=dev)
    tally.reset(E)
    loop = GraphedLoop(stream(tally.step), unroll=T, warmup=1, device=dev)

    def replay():
        tally.reset(E)
        loop.replay()

    us = _time_replays(replay, replays)
    filled = E - tally.remaining()
    if filled != (0 if variant == "idle" else T * PER_STEP):
        sys.exit(f"{variant}: {filled} records behind a replay, not the {T * PER_STEP} its stream appends")
    return us


def _reward(obs, info):
    import torch

    return torch.abs(obs[:, 0]).neg_().add_(1.0)


def _setup(n):
    N = n
    import torch
    import torch.nn as nn

    import upkie_amd.envs as envs
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    env = envs.make("Upkie-HIP-Pendulum-Vec", num_envs=N, frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=LIMIT)
    dev = env.device
    tower = lambda: nn.Sequential(nn.Linear(4, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)  # noqa: E731
    policy = MlpActorCritic.from_modules(tower(), tower(), nn.Parameter(torch.zeros(1, device=dev)), action_low=[-1.0], action_high=[1.0])
    return env, policy


def _eval_step(variant, replays, n):
    E = n
    from upkie_amd.evaluation import PolicyEvaluator
    from upkie_amd.graphs import GraphedLoop

    env, policy = _setup(n)
    with env:
        runner = PolicyEvaluator(policy, env, E, reward_fn=_reward, graph=False)
        runner.begin(E, 0)
        step = runner.step if variant == "step" else (lambda: runner.step(record=False))
        loop = GraphedLoop(step, unroll=T, warmup=1, device=env.device)
        return _time_replays(loop.replay, replays)


def _evaluate(replays, n):
    E = n
    import torch

    from upkie_amd.evaluation import PolicyEvaluator

    env, policy = _setup(n)
    with env:
        runner = PolicyEvaluator(policy, env, E, reward_fn=_reward, chunk=32, graph=True)
        runner.run(E, seed=0)  # (captures)
        torch.cuda.synchronize()
        begin = time.perf_counter()
        for k in range(replays):
            result = runner.run(E, seed=0)
        torch.cuda.synchronize()
        return (time.perf_counter() - begin) * 1e3 / replays, result


def _torch_loop(replays, n):
    """SB3's loop with the env, the policy and the reward on the device and the bookkeeping as torch ops: the finished
    envs under quota are gathered on the host every step."""
    N = E = n
    import torch

    env, policy = _setup(n)
    with env:
        dev = env.device
        action = torch.empty(N, 1, device=dev)
        targets = (E + torch.arange(N, device=dev)) // N

        def evaluate():
            env.reset(seed=0)
            obs = env.observation
            returns, lengths = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
            counts = torch.zeros(N, dtype=torch.int64, device=dev)
            rewards, ep_lengths = [], []
            while len(rewards) < E:
                policy.mean_action(obs, action)
                obs, _, terminated, truncated, info = env.step(action)
                live = counts < targets
                returns += torch.where(live, _reward(obs, info).double(), 0.0)
                lengths += live
                idx = torch.nonzero(live & (terminated | truncated)).reshape(-1)  # (the host synchronisation)
                if idx.numel():
                    rewards += returns[idx].tolist()
                    ep_lengths += lengths[idx].tolist()
                    counts[idx] += 1
                    returns[idx], lengths[idx] = 0.0, 0
            return rewards, ep_lengths

        evaluate()
        torch.cuda.synchronize()
        begin = time.perf_counter()
        for _ in range(replays):
            rewards, ep_lengths = evaluate()
        torch.cuda.synchronize()
        return (time.perf_counter() - begin) * 1e3 / replays, {"episode_rewards": rewards, "episode_lengths": ep_lengths}


def measure(variant, replays, n):
    E = n
    line = {"variant": variant, "num_envs": n, "n_eval_episodes": E, "replays": replays}
    if variant in ("tally", "idle", "episodes"):
        line["us_per_step"] = round(_bookkeeping(variant, replays, n), 3)
    elif variant in ("step", "no_tally"):
        line["us_per_step"] = round(_eval_step(variant, replays, n), 3)
    else:
        ms, result = _evaluate(replays, n) if variant == "evaluate" else _torch_loop(replays, n)
        line["ms_per_evaluation"] = round(ms, 3)
        line["mean_ep_length"] = sum(result["episode_lengths"]) / E
        line["mean_reward"] = sum(result["episode_rewards"]) / E
    print(json.dumps(line), flush=True)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--replays", type=int, default=400)
    parser.add_argument("--variant", choices=VARIANTS)
    parser.add_argument("--out", help="append the result lines to this file")
    parser.add_argument("--num-envs", type=int, default=DEFAULT_ENVS, help="envs, and episodes asked for")
    args = parser.parse_args()
    N = args.num_envs
    if N <= T * PER_STEP:
        parser.error(f"--num-envs must be above {T * PER_STEP}: the tally's stream ends {PER_STEP} other envs on each of {T} steps and must not fill the list")
    if args.variant:
        measure(args.variant, args.replays, N)
        return
    samples = {v: [] for v in VARIANTS}
    used = {v: args.replays if v not in UNITS else max(1, args.replays // 10) for v in VARIANTS}
    for _ in range(args.rounds):
        for variant in VARIANTS:
            replays = used[variant]
            cmd = [sys.executable, os.path.abspath(__file__), "--variant", variant, "--replays", str(replays), "--num-envs", str(N)]
            result = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if result.returncode != 0:
                sys.exit(f"{variant} failed ({result.returncode}):\n{result.stderr[-2000:]}")
            samples[variant].append(json.loads(result.stdout.strip().splitlines()[-1])[UNITS.get(variant, "us_per_step")])
    lines = []
    for variant, values in samples.items():
        unit = UNITS.get(variant, "us_per_step")
        lines.append({"variant": variant, f"{unit}_median": round(statistics.median(values), 3), "min": min(values), "max": max(values),
                      "rounds": args.rounds, "replays": used[variant], "num_envs": N, "n_eval_episodes": N})
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
