"""The time-limit bootstrap (`MlpActorCritic.bootstrap_time_limits`) and the episode statistics (`EpisodeStatistics`),
timed with device events after a warm-up:

  (a) the bootstrap launch at N in {4096, 65536}, [64, 64] and [256, 256] critics, with no env, one env in 400 and every
      env truncating; beside it the torch composition `policy.value(final_obs)` + mask / mul / add;
  (b) the statistics launch at N in {4096, 65536, 1048576}, window 100 and 1000, one env in 400 ending per step;
  (c) the graphed 4096-env rollout step of examples/ppo_mlp_normalized_rollout.py (MlpActorCritic + env.step +
      RunningNormalizer + buffer writes, `GraphedLoop` of 16 steps) without and with both launches.

Eager and graphed times are host-clock-free: device events around the window (graphed: 16 launches per replay).
Prints one JSON line per measurement. Kernel times: `--profile` runs each launch of (a) and (b) alone, `--steps` times
per configuration, configurations separated by a fill kernel, for `rocprofv3 --kernel-trace --stats`; `--summarize
DIR` then prints one JSON line per configuration from the kernel trace under DIR (the launches are
mlp_bootstrap_time_limits_kernel<W, ACT> and episodes_step_kernel).

usage: python tools/bench_time_limits.py [--steps 2000] [--warmup 200] [--part a|b|c|abc] [--profile] [--summarize DIR]"""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SLOTS = 16
DEV = "cuda:0"


def time_us(fn, steps, warmup, per_call=1):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / (steps * per_call)


def _policy(width):
    import torch
    import torch.nn as nn

    from upkie_amd.policies import MlpActorCritic

    torch.manual_seed(0)
    tower = lambda: nn.Sequential(nn.Linear(4, width), nn.Tanh(), nn.Linear(width, width), nn.Tanh(), nn.Linear(width, 1)).to(DEV)  # noqa: E731
    return MlpActorCritic.from_modules(tower(), tower(), torch.zeros(1, device=DEV), [-1.0], [1.0], obs_mean=[0.0] * 4, obs_var=[1.0] * 4)


def _bootstrap_configs():
    for width in (64, 256):
        for n in (4096, 65536):
            for pattern in ("none", "1/400", "all"):
                yield width, n, pattern


def _flags(n, pattern):
    import torch

    term = torch.zeros(n, dtype=torch.bool, device=DEV)
    trunc = torch.zeros(n, dtype=torch.bool, device=DEV)
    if pattern == "all":
        trunc[:] = True
    elif pattern == "1/400":
        trunc[::400] = True
    return term, trunc


def _stats_configs():
    for n in (4096, 65536, 1048576):
        for window in (100, 1000):
            yield n, window


def part_a(args):
    import torch

    from upkie_amd.graphs import GraphedLoop

    for width, n, pattern in _bootstrap_configs():
        pol = _policy(width)
        final_obs = torch.randn(n, 4, device=DEV)
        reward = torch.randn(n, device=DEV)
        term, trunc = _flags(n, pattern)
        gamma_f32 = torch.tensor(0.99, dtype=torch.float32, device=DEV)
        mask = trunc & ~term
        kernel = lambda: pol.bootstrap_time_limits(final_obs, term, trunc, reward, 0.99)  # noqa: E731

        def composed():
            v = pol.value(final_obs)  # (the policy's own value buffer)
            torch.where(mask, reward + gamma_f32 * v, reward, out=reward)

        row = {"part": "a", "what": "time-limit bootstrap", "num_envs": n, "critic": [width, width], "truncating": pattern}
        for name, fn in (("kernel", kernel), ("torch", composed)):
            row[f"{name}_us_eager"] = round(time_us(fn, args.steps, args.warmup), 2)
            loop = GraphedLoop(fn, unroll=SLOTS)
            row[f"{name}_us_graphed"] = round(time_us(loop.replay, max(args.steps // SLOTS, 1), max(args.warmup // SLOTS, 1), SLOTS), 2)
        print(json.dumps(row), flush=True)


def _stats_body(n, window):
    import torch

    from upkie_amd.episodes import EpisodeStatistics

    stats = EpisodeStatistics(n, window=window, device=DEV)
    reward = torch.randn(n, device=DEV)
    term = torch.zeros(n, dtype=torch.bool, device=DEV)
    trunc = torch.zeros(n, dtype=torch.bool, device=DEV)
    trunc[::400] = True
    return lambda: stats.step(reward, term, trunc)


def part_b(args):
    from upkie_amd.graphs import GraphedLoop

    for n, window in _stats_configs():
        body = _stats_body(n, window)
        eager = time_us(body, args.steps, args.warmup)
        loop = GraphedLoop(body, unroll=SLOTS)
        graphed = time_us(loop.replay, max(args.steps // SLOTS, 1), max(args.warmup // SLOTS, 1), SLOTS)
        print(json.dumps({"part": "b", "what": "episode statistics step (one env in 400 ends per step)", "num_envs": n, "window": window,
                          "us_eager": round(eager, 2), "us_graphed": round(graphed, 2)}), flush=True)


def part_c(args):
    import torch
    import torch.nn as nn

    import upkie_amd.envs as envs
    from upkie_amd.episodes import EpisodeStatistics
    from upkie_amd.graphs import GraphedLoop
    from upkie_amd.normalize import RunningNormalizer
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.rollout import RolloutBuffer
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    n = 4096
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    results = {}
    for form in ("without", "with", "without", "with"):  # (alternated: the spread shows in the two pairs)
        with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=n, frequency=200.0, init_state=init, autoreset_mode="same_step",
                       max_episode_steps=400) as env:
            dev = env.device
            torch.manual_seed(0)
            tower = lambda: nn.Sequential(nn.Linear(4, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)  # noqa: E731
            policy = MlpActorCritic.from_modules(tower(), tower(), torch.zeros(1, device=dev), [-1.0], [1.0])
            norm = RunningNormalizer.for_env(env)
            norm.attach(policy)
            stats = EpisodeStatistics(n, device=dev) if form == "with" else None
            buf = RolloutBuffer(SLOTS, n, obs_shape=(4,), action_shape=(1,), device=dev)
            env.reset(seed=0)
            obs = env.observation
            norm.reset(obs)
            env_action = torch.empty(n, 1, device=dev)
            reward = torch.empty(n, device=dev)
            starts = torch.zeros(n, dtype=torch.uint8, device=dev)
            slot = {"t": 0}

            def body():
                t = slot["t"]
                buf.episode_starts[t].copy_(starts)
                policy.act(obs, out={"norm_obs": buf.observations[t], "action": buf.actions[t], "value": buf.values[t],
                                     "log_prob": buf.log_probs[t], "env_action": env_action})
                next_obs, _, terminated, truncated, info = env.step(env_action)
                torch.abs(next_obs[:, 0], out=reward).neg_().add_(1.0)
                if stats is not None:
                    stats.step(reward, terminated, truncated)
                norm.step(next_obs, reward, terminated, truncated, out={"reward": buf.rewards[t], "episode_starts": starts})
                if stats is not None:
                    policy.bootstrap_time_limits(info["final_obs"], terminated, truncated, buf.rewards[t], buf.gamma)
                slot["t"] = (t + 1) % SLOTS

            loop = GraphedLoop(body, unroll=SLOTS)
            graphed = time_us(loop.replay, max(args.steps // SLOTS, 1), max(args.warmup // SLOTS, 1), SLOTS)
            results.setdefault(form, []).append(graphed)
            print(json.dumps({"part": "c", "what": f"graphed rollout step (policy + env.step + RunningNormalizer), {form} bootstrap and "
                              "episode statistics", "num_envs": n, "us_per_step_graphed": round(graphed, 2)}), flush=True)
    added = [w - o for w, o in zip(results["with"], results["without"])]
    print(json.dumps({"part": "c", "what": "added by the two launches (graphed step with minus without, per pair)", "num_envs": n,
                      "us": [round(x, 2) for x in added]}), flush=True)


def profile(args):
    """Each launch of (a) and (b) alone, `--steps` times per configuration, a fill kernel between configurations."""
    import torch

    sep = torch.zeros(1, device=DEV)
    for width, n, pattern in _bootstrap_configs():
        pol = _policy(width)
        final_obs, reward = torch.randn(n, 4, device=DEV), torch.randn(n, device=DEV)
        term, trunc = _flags(n, pattern)
        for _ in range(args.steps):
            pol.bootstrap_time_limits(final_obs, term, trunc, reward, 0.99)
        sep.fill_(1.0)
        torch.cuda.synchronize()
    for n, window in _stats_configs():
        body = _stats_body(n, window)
        for _ in range(args.steps):
            body()
        sep.fill_(1.0)
        torch.cuda.synchronize()


def summarize(directory):
    """One JSON line per configuration of `profile` from the kernel trace under `directory`: the runs of consecutive
    dispatches of the same kernel, in dispatch order, matched to the configurations in the order `profile` ran them."""
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        sys.exit(f"bench_time_limits: no kernel trace under {directory}")
    rows = []
    for path in paths:
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    runs, current = [], None
    for r in rows:
        name = r["Kernel_Name"]
        ours = "bootstrap_time_limits" in name or "episodes_step_kernel" in name
        if not ours:
            current = None
            continue
        if current is None or current["name"] != name:
            current = {"name": name, "ns": []}
            runs.append(current)
        current["ns"].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    configs = [{"launch": "bootstrap", "critic": [w, w], "num_envs": n, "truncating": p} for w, n, p in _bootstrap_configs()]
    configs += [{"launch": "episode statistics", "num_envs": n, "window": w, "ending": "1/400"} for n, w in _stats_configs()]
    if len(runs) != len(configs):
        sys.exit(f"bench_time_limits: {len(runs)} runs of our kernels in the trace, {len(configs)} configurations")
    for cfg, run in zip(configs, runs):
        ns = sorted(run["ns"][len(run["ns"]) // 10:])  # (the first tenth: warm-up)
        cfg.update({"kernel": run["name"].split("(")[0], "dispatches": len(run["ns"]), "median_us": round(ns[len(ns) // 2] / 1e3, 2),
                    "mean_us": round(sum(ns) / len(ns) / 1e3, 2), "source": "rocprofv3 --kernel-trace"})
        print(json.dumps(cfg), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--part", default="abc")
    ap.add_argument("--profile", action="store_true", help="launches of (a) and (b) alone, for rocprofv3 --kernel-trace")
    ap.add_argument("--summarize", metavar="DIR", help="per-configuration kernel times from a --profile trace under DIR")
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize)
        sys.exit(0)
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_time_limits: no HIP device (there is no CPU fallback)")
    if args.profile:
        profile(args)
        sys.exit(0)
    if "a" in args.part:
        part_a(args)
    if "b" in args.part:
        part_b(args)
    if "c" in args.part:
        part_c(args)
