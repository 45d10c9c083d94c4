"""The running normaliser (`upkie_amd.normalize.RunningNormalizer`) and the rollout step around it, timed with device
events after a warm-up:

  (a) the normalizer step alone (training, norm_obs and norm_reward: two launches) at N in {4096, 16384, 65536,
      1048576} and obs_dim D in {4, 30}, eager and replayed from a hipGraph (16 steps per replay);
  (b) a graphed rollout step at N = 4096 (`GraphedLoop`, 16 steps per replay) -- MlpActorCritic + env.step + buffer
      writes -- without normalization, with this normalizer, and with the same VecNormalize semantics as torch ops.

Prints one JSON line per measurement. Kernel times: run under `rocprofv3 --kernel-trace --stats` (the launches are
vecnorm_moments_kernel and vecnorm_apply_kernel).

usage: python tools/bench_vecnorm.py [--steps 2000] [--warmup 200] [--part a|b|ab]"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import upkie_amd.envs as envs  # noqa: E402
from upkie_amd.graphs import GraphedLoop  # noqa: E402
from upkie_amd.normalize import RunningNormalizer, packed_offsets  # noqa: E402
from upkie_amd.policies import MlpActorCritic  # noqa: E402
from upkie_amd.rollout import RolloutBuffer  # noqa: E402
from upkie_amd.utils.robot_state import RobotState  # noqa: E402
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization  # noqa: E402

SLOTS = 16


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
    for d in (4, 30):
        for n in (4096, 16384, 65536, 1048576):
            norm = RunningNormalizer(n, d, device=dev)
            obs = torch.randn(n, d, device=dev)
            reward = torch.randn(n, device=dev)
            term = torch.rand(n, device=dev) < 0.01
            trunc = torch.zeros(n, dtype=torch.bool, device=dev)
            out = {"episode_starts": torch.empty(n, dtype=torch.uint8, device=dev)}
            body = lambda: norm.step(obs, reward, term, trunc, out=out)  # noqa: E731
            eager = time_us(body, args.steps, args.warmup)
            loop = GraphedLoop(body, unroll=SLOTS)
            graphed = time_us(loop.replay, max(args.steps // SLOTS, 1), max(args.warmup // SLOTS, 1), per_call=SLOTS)
            print(json.dumps({"part": "a", "what": "normalizer step (moments + apply launches), event-timed", "num_envs": n, "obs_dim": d,
                              "us_per_step_eager": round(eager, 2), "us_per_step_graphed": round(graphed, 2)}), flush=True)


class TorchVecNormalize:
    """The same semantics as torch ops (fp64 state, float32 outputs), writing the policy's packed statistics too."""

    def __init__(self, n, d, policy, dev, gamma=0.99, eps=1e-8, clip_obs=10.0, clip_reward=10.0):
        f64 = dict(dtype=torch.float64, device=dev)
        self.mean, self.var, self.count = torch.zeros(d, **f64), torch.ones(d, **f64), torch.full((), 1e-4, **f64)
        self.rmean, self.rvar, self.rcount = torch.zeros((), **f64), torch.ones((), **f64), torch.full((), 1e-4, **f64)
        self.returns = torch.zeros(n, **f64)
        self.policy, self.d, self.n = policy, d, n
        self.gamma, self.eps, self.clip_obs, self.clip_reward = gamma, eps, clip_obs, clip_reward

    def _update(self, mean, var, count, x):
        bm, bv = x.mean(0), x.var(0, unbiased=False)
        delta = bm - mean
        tot = count + self.n
        var.copy_((var * count + bv * self.n + delta * delta * count * self.n / tot) / tot)
        mean.add_(delta * self.n / tot)
        count.copy_(tot)

    def step(self, obs, reward, terminated, truncated, reward_out, starts_out):
        self._update(self.mean, self.var, self.count, obs.double())
        r = reward.double()
        self.returns.mul_(self.gamma).add_(r)
        self._update(self.rmean, self.rvar, self.rcount, self.returns)
        torch.clamp(r / torch.sqrt(self.rvar + self.eps), -self.clip_reward, self.clip_reward, out=r)
        reward_out.copy_(r)
        done = torch.logical_or(terminated, truncated)
        self.returns.masked_fill_(done, 0.0)
        starts_out.copy_(done)
        mean_at, std_at = packed_offsets(self.d)
        self.policy.packed[mean_at: mean_at + self.d].copy_(self.mean)
        self.policy.packed[std_at: std_at + self.d].copy_(torch.sqrt(self.var + self.eps))


def part_b(args):
    n = 4096
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    results = {}
    for form in ("no normalization", "RunningNormalizer", "torch ops"):
        with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=n, frequency=200.0, init_state=init, autoreset_mode="same_step",
                       max_episode_steps=400) as env:
            dev = env.device
            env.reset(seed=0)
            obs = env.observation
            torch.manual_seed(0)
            actor = nn.Sequential(nn.Linear(4, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)
            critic = nn.Sequential(nn.Linear(4, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)
            policy = MlpActorCritic.from_modules(actor, critic, torch.zeros(1, device=dev), [-1.0], [1.0],
                                                 obs_mean=None if form == "no normalization" else [0.0] * 4)
            norm = RunningNormalizer.for_env(env) if form == "RunningNormalizer" else None
            twin = TorchVecNormalize(n, 4, policy, dev) if form == "torch ops" else None
            if norm is not None:
                norm.attach(policy)
            buf = RolloutBuffer(SLOTS, n, obs_shape=(4,), action_shape=(1,), device=dev)
            env_action = torch.empty(n, 1, device=dev)
            starts = torch.zeros(n, dtype=torch.uint8, device=dev)
            slot = {"t": 0}

            def body():
                t = slot["t"]
                policy.act(obs, out={"norm_obs": buf.observations[t], "action": buf.actions[t], "value": buf.values[t],
                                     "log_prob": buf.log_probs[t], "env_action": env_action})
                next_obs, reward, terminated, truncated, _ = env.step(env_action)
                if norm is not None:
                    norm.step(next_obs, reward, terminated, truncated, out={"reward": buf.rewards[t], "episode_starts": starts})
                elif twin is not None:
                    twin.step(next_obs, reward, terminated, truncated, buf.rewards[t], starts)
                else:
                    buf.rewards[t].copy_(reward)
                    torch.logical_or(terminated, truncated, out=starts)
                slot["t"] = (t + 1) % SLOTS

            loop = GraphedLoop(body, unroll=SLOTS)
            graphed = time_us(loop.replay, max(args.steps // SLOTS, 1), max(args.warmup // SLOTS, 1), per_call=SLOTS)
            results[form] = graphed
            print(json.dumps({"part": "b", "what": f"graphed rollout step: MlpActorCritic + env.step + buffer, {form}", "num_envs": n,
                              "us_per_step_graphed": round(graphed, 2)}), flush=True)
    base = results["no normalization"]
    print(json.dumps({"part": "b", "what": "added by normalization (graphed step minus the step without it)", "num_envs": n,
                      "running_normalizer_us": round(results["RunningNormalizer"] - base, 2),
                      "torch_ops_us": round(results["torch ops"] - base, 2)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--part", default="ab")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_vecnorm: no HIP device (there is no CPU fallback)")
    if "a" in args.part:
        part_a(args)
    if "b" in args.part:
        part_b(args)
