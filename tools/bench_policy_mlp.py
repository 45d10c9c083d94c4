"""The MLP actor-critic launch (`upkie_amd.policies.MlpActorCritic`) and the rollout step around it, timed with device
events after a warm-up:

  (a) the policy launch alone (obs 4, act 1, sampled) at N in {4096, 16384, 65536}, towers [64, 64] and [256, 256];
  (b) a full rollout step at N = 4096 -- env.step + policy + rollout-buffer writes -- with the one-launch policy and
      with the same modules as torch ops (+ torch.distributions.Normal), each eager and replayed from a hipGraph
      (`GraphedLoop`, 16 steps per replay); env.step alone, eager and graphed, as the baseline.

Prints one JSON line per measurement; the FLOP count comes from the shapes, and the share of the fp32 MFMA peak
(157.3 TFLOP/s) is of a latency-bound launch, not of a compute-bound one. Kernel times: run under
`rocprofv3 --kernel-trace --stats` (the launch is mlp_actor_critic_kernel<W, ACT>).

usage: python tools/bench_policy_mlp.py [--steps 2000] [--warmup 200] [--part a|b|ab]"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import upkie_amd.envs as envs  # noqa: E402
from upkie_amd.graphs import GraphedLoop  # noqa: E402
from upkie_amd.policies import MlpActorCritic  # noqa: E402
from upkie_amd.rollout import RolloutBuffer  # noqa: E402
from upkie_amd.utils.robot_state import RobotState  # noqa: E402
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization  # noqa: E402

PEAK_FP32 = 157.3e12  # MFMA f32 (= vector) peak, FLOP/s


def tower(d_in, widths, d_out):
    mods, n = [], d_in
    for w in widths:
        mods += [nn.Linear(n, w), nn.Tanh()]
        n = w
    return nn.Sequential(*mods, nn.Linear(n, d_out))


def flops_per_env(d_in, widths, d_out):
    dims = [d_in] + list(widths) + [d_out]
    return sum(2 * a * b for a, b in zip(dims[:-1], dims[1:]))


def time_us(fn, steps, warmup, per_call=1):
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


def part_a(args):
    dev = "cuda:0"
    for widths in ([64, 64], [256, 256]):
        torch.manual_seed(0)
        actor, critic = tower(4, widths, 1).to(dev), tower(4, widths, 1).to(dev)
        for n in (4096, 16384, 65536):
            policy = MlpActorCritic.from_modules(actor, critic, torch.zeros(1, device=dev), [-1.0], [1.0])  # (one batch size per policy)
            obs = torch.randn(n, 4, device=dev)
            us = time_us(lambda: policy.act(obs), args.steps, args.warmup)
            flop = n * (flops_per_env(4, widths, 1) * 2)
            print(json.dumps({"part": "a", "what": "policy launch, eager, event-timed (includes launch overhead)", "num_envs": n,
                              "towers": widths, "us_per_call": round(us, 2), "flop": flop,
                              "share_of_fp32_mfma_peak_latency_bound": round(flop / (us * 1e-6) / PEAK_FP32, 5)}), flush=True)


def part_b(args):
    n, slots = 4096, 16
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=n, frequency=200.0, init_state=init, autoreset_mode="same_step",
                   max_episode_steps=400) as env:
        dev = env.device
        obs, _ = env.reset(seed=0)
        obs = env.observation
        torch.manual_seed(0)
        actor, critic = tower(4, [64, 64], 1).to(dev), tower(4, [64, 64], 1).to(dev)
        log_std = torch.zeros(1, device=dev)
        policy = MlpActorCritic.from_modules(actor, critic, log_std, [-1.0], [1.0])
        buf = RolloutBuffer(slots, n, obs_shape=(4,), action_shape=(1,), device=dev)
        fixed_action = torch.zeros(n, 1, device=dev)
        env_action = torch.empty(n, 1, device=dev)
        slot = {"t": 0}

        def step_only():
            env.step(fixed_action)

        def ours():
            t = slot["t"]
            policy.act(obs, out={"norm_obs": buf.observations[t], "action": buf.actions[t], "value": buf.values[t], "log_prob": buf.log_probs[t],
                                 "env_action": env_action})
            _, reward, terminated, truncated, _ = env.step(env_action)
            buf.rewards[t].copy_(reward)
            torch.logical_or(terminated, truncated, out=buf.episode_starts[t])
            slot["t"] = (t + 1) % slots

        def torch_modules():
            t = slot["t"]
            with torch.no_grad():
                mean = actor(obs)
                value = critic(obs)[:, 0]
                dist = torch.distributions.Normal(mean, log_std.exp(), validate_args=False)  # (validation syncs: not capturable)
                action = mean + log_std.exp() * torch.randn_like(mean)  # (dist.rsample(): the same draw)
                log_prob = dist.log_prob(action).sum(-1)
                buf.observations[t].copy_(obs)
                buf.actions[t].copy_(action)
                buf.values[t].copy_(value)
                buf.log_probs[t].copy_(log_prob)
                _, reward, terminated, truncated, _ = env.step(action.clamp(-1.0, 1.0))
                buf.rewards[t].copy_(reward)
                torch.logical_or(terminated, truncated, out=buf.episode_starts[t])
            slot["t"] = (t + 1) % slots

        results = {}
        for name, body in (("env.step alone", step_only), ("env.step + MlpActorCritic + buffer", ours),
                           ("env.step + torch modules + Normal + buffer", torch_modules)):  # (the torch body last: a failed capture ends the part)
            eager = time_us(body, args.steps, args.warmup)
            try:
                loop = GraphedLoop(body, unroll=slots)
                graphed = time_us(loop.replay, max(args.steps // slots, 1), max(args.warmup // slots, 1), per_call=slots)
            except RuntimeError as exc:  # (torch's Normal.sample could not be captured on every torch build)
                print(json.dumps({"part": "b", "what": name, "graph_capture_failed": str(exc).splitlines()[0]}), flush=True)
                graphed = float("nan")
            results[name] = (eager, graphed)
            print(json.dumps({"part": "b", "what": name, "num_envs": n, "towers": [64, 64], "us_per_step_eager": round(eager, 2),
                              "us_per_step_graphed": round(graphed, 2)}), flush=True)
        base, ours_t, torch_t = (results[k] for k in results)
        print(json.dumps({"part": "b", "what": "policy side of a rollout step (loop minus env.step alone)", "num_envs": n,
                          "mlp_actor_critic_eager_us": round(ours_t[0] - base[0], 2), "mlp_actor_critic_graphed_us": round(ours_t[1] - base[1], 2),
                          "torch_eager_us": round(torch_t[0] - base[0], 2), "torch_graphed_us": round(torch_t[1] - base[1], 2)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--part", default="ab")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_policy_mlp: no HIP device (there is no CPU fallback)")
    if "a" in args.part:
        part_a(args)
    if "b" in args.part:
        part_b(args)
