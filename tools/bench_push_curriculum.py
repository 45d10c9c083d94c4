"""What the push curriculum (`upkie_amd.events.PushLevels`, ``live=True``) costs at 4096 envs (`--num-envs N`: at N) next
to the plain events launch, MEASURED IN THE SAME PROCESS: three stages -- the old entry point, the new one with one level
(``live=True``, L = 0) and the new one with L = 8 -- on handles of their own, whose graph replays of 128 steps alternate,
so that a drift of the clocks reaches all three alike. Time per env step, device events around whole replays, of

  launch          the events launch alone, pushes only (tools/bench_episode_events.py's `pushes`), on handles that are
                  never stepped: nobody ends (`us_old`, `us_live`, `us_levels`);
  ends            the launch with per-episode inertias on the pendulum workload's own ends of episodes
                  (tools/bench_episode_events.py's `redraw`: the same recorded flags);
  counts          the level histogram (`level_counts`: a memset and a launch) at L = 8;
  rollout         one graphed `Ppo` rollout step under the plain events and under the levelled, live ones, two `Ppo`
                  objects whose replays alternate: `us_old`, `us_levels`, `us_added` the difference.

Each measurement is a child process; the parent interleaves the variants over `--rounds` rounds and prints, per variant,
one JSON line with the median and the spread (min, max) over the rounds: the spread of `us_old` is what a difference has
to exceed to be one. `--variant NAME` runs one measurement in this process.

usage: python tools/bench_push_curriculum.py [--rounds 3] [--replays 100] [--variant NAME] [--num-envs 4096] [--out profiles/push_curriculum_bench.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_episode_events as base  # noqa: E402  (the env, the policy, the recorded flags' stretch, the timing loop)

T, PUSHES = base.T, base.PUSHES
VARIANTS = ("launch", "ends", "counts", "rollout")
LEVELS = 8
CHUNKS = 8  # alternations per measurement


def _alternate(replays_of, replays):
    """``{name: replay}`` -> ``{name: median us per step}`` over CHUNKS alternating chunks."""
    chunk = max(1, replays // CHUNKS)
    samples = {name: [] for name in replays_of}
    for _ in range(CHUNKS):
        for name, replay in replays_of.items():
            samples[name].append(base._time_replays(replay, chunk))
    return {name: round(statistics.median(values), 3) for name, values in samples.items()}


def _curriculum():
    from upkie_amd.events import PushLevels

    return PushLevels(LEVELS, start=0, up=1, down=2, min_pushes=1)


def _stages(n, variation):
    """The three stages, each on a handle of its own that is never stepped."""
    from upkie_amd import abi
    from upkie_amd.events import EpisodeEvents
    from upkie_amd.model.model import Model
    from upkie_amd.sim import BatchedSim

    model = Model()
    stages = {}
    for name, kw in (("us_old", {}), ("us_live", dict(live=True)), ("us_levels", dict(curriculum=_curriculum()))):
        sim = BatchedSim(abi.default_sim_config(n), model.struct)
        env = types.SimpleNamespace(sim=sim, model=model, num_envs=n, device=sim.device)
        stages[name] = EpisodeEvents(env, inertia_variation=variation, **PUSHES, **kw)
    return stages


def _workload_flags(n, terminated, truncated):
    """tools/bench_episode_events.py's `redraw` flags: steps 337-464 of the pendulum env under the untrained policy."""
    import torch

    env, policy = base._setup(n)
    with env:
        action = torch.empty(n, 1, device=terminated.device)
        env.reset(seed=0)
        obs = env.observation
        for t in range(base.LEAD_IN + T):
            policy.mean_action(obs, action)
            obs, _, term, trunc, _ = env.step(action)
            if t >= base.LEAD_IN:
                terminated[t - base.LEAD_IN].copy_(term)
                truncated[t - base.LEAD_IN].copy_(trunc)
        torch.cuda.synchronize()
    ended = (terminated | truncated).float()
    return {"finish_rate": round(float(ended.mean()), 6), "finish_peak": round(float(ended.mean(dim=1).max()), 6)}


def _launch_alone(variant, replays, n):
    import torch

    from upkie_amd.graphs import GraphedLoop

    dev = "cuda:0"
    terminated = torch.zeros(T, n, dtype=torch.bool, device=dev)
    truncated = torch.zeros(T, n, dtype=torch.bool, device=dev)
    extra = _workload_flags(n, terminated, truncated) if variant == "ends" else {}
    stages = _stages(n, 0.2 if variant == "ends" else 0.0)
    loops = {}
    for name, events in stages.items():
        slot = {"t": T - 1}  # (the capture's one warm-up step takes the last slot: the captured steps are 0 .. T - 1)

        def body(events=events, slot=slot):
            t = slot["t"]
            events.step(terminated[t], truncated[t])
            slot["t"] = (t + 1) % T

        loops[name] = GraphedLoop(body, unroll=T, warmup=1, device=dev).replay
    line = _alternate(loops, replays)
    line["us_levels_minus_old"] = round(line["us_levels"] - line["us_old"], 3)
    levelled = stages["us_levels"]
    extra["pushes_per_env_step"] = round(float(levelled.pushes.sum()) / float(int(levelled.calls[0]) * n), 6)
    extra["level_mean"] = round(float(levelled.level.float().mean()), 4)
    return {**line, **extra}


def _counts(replays, n):
    import torch

    from upkie_amd.graphs import GraphedLoop

    events = _stages(n, 0.0)["us_levels"]
    events.set_levels(torch.arange(n, dtype=torch.int32) % (LEVELS + 1))
    loop = GraphedLoop(events.level_counts, unroll=T, warmup=1, device="cuda:0")
    us = base._time_replays(loop.replay, replays)
    assert int(events.level_counts().sum()) == n
    return {"us_per_call": round(us, 3)}


def _rollout(replays, n):
    env_a, plain = base._ppo(n, dict(inertia_variation=0.2, **PUSHES))
    env_b, levelled = base._ppo(n, dict(inertia_variation=0.2, curriculum=_curriculum(), live=True, **PUSHES))
    with env_a, env_b:
        line = _alternate({"us_old": plain._loop.replay, "us_levels": levelled._loop.replay}, replays)
        line["us_added"] = round(line["us_levels"] - line["us_old"], 3)
        line["level_mean"] = round(float(levelled.events.level.float().mean()), 4)
        return line


def measure(variant, replays, n):
    line = {"variant": variant, "num_envs": n, "replays": replays, "levels": LEVELS}
    if variant in ("launch", "ends"):
        line.update(_launch_alone(variant, replays, n))
    else:
        line.update(_counts(replays, n) if variant == "counts" else _rollout(replays, n))
    print(json.dumps(line), flush=True)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--replays", type=int, default=100)
    parser.add_argument("--variant", choices=VARIANTS)
    parser.add_argument("--out", help="append the result lines to this file")
    parser.add_argument("--num-envs", type=int, default=base.DEFAULT_ENVS)
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
            print(f"round {len(samples[variant])}: {result.stdout.strip().splitlines()[-1]}", file=sys.stderr, flush=True)
    lines = []
    for variant, runs in samples.items():
        line = {"variant": variant, "rounds": args.rounds, "replays": args.replays, "num_envs": args.num_envs, "levels": LEVELS}
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
