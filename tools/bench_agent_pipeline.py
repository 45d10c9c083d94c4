"""What the agent pipeline (`upkie_amd.pipeline.AgentPipeline`: action shaping, noise, frame stacking) costs inside
`Ppo`'s graphed 128-step rollout at 4096 envs, K = 8, D = 4, A = 1, every stage switched on. Time per rollout step,
device events around whole replays, of

  none     `Ppo` without a pipeline (the 4-word observation; the code path of a `Ppo` built before the pipeline existed);
  none40   the same with the env's observation widened to 40 words by one strided copy per step (what the policy, the
           normaliser and the bootstrap pay for 40 words instead of 4, plus that copy launch);
  kernels  `Ppo(pipeline=AgentPipeline(...))`: two launches per step;
  torch    the same semantics as torch ops inside the same captured step (`TorchPipeline` below: a roll, masked
           writes and a concatenation for the stack, ``torch.randn`` for the noise, which is not keyed per env).

Each measurement is a child process; the parent interleaves the variants over `--rounds` rounds and prints, per variant,
the median and the spread (min, max) over the rounds, then the differences. `--check` compares `TorchPipeline` with the
kernels, noise off, over a scripted sequence (a third witness of the semantics beside the numpy twin and the deque of
tests/agent_pipeline_reference.py): bit for bit where the data only moves, to 4 * 2^-24 on the commands.
`--only-kernels` runs the kernels variant alone in this process for ``rocprofv3 --kernel-trace --stats``.

usage: python tools/bench_agent_pipeline.py [--rounds 5] [--replays 20] [--check] [--only-kernels] [--variant NAME]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, K, D, A, T = 4096, 8, 4, 1, 128
DT, LAG, SIGMA_A, SIGMA_O = 1.0 / 200.0, 0.05, [0.02], [0.002, 0.002, 0.01, 0.01]
VARIANTS = ("none", "none40", "kernels", "torch")


class TorchPipeline:
    """`AgentPipeline`'s interface and semantics as torch ops on persistent tensors (capturable). The noise comes from
    ``torch.randn``: one generator for the batch, not keyed per env."""

    def __init__(self, num_envs, obs_dim, low, high, dt, stack=8, integrate_action=False, action_noise=None, action_lag=None,
                 observation_noise=None, device="cuda:0"):
        import torch

        self.num_envs, self.obs_dim, self.act_dim, self.stack = num_envs, obs_dim, len(low), stack
        self.frame_dim = obs_dim + self.act_dim
        self.stacked_dim = stack * self.frame_dim
        f32 = dict(dtype=torch.float32, device=device)
        self.low, self.high = torch.tensor(low, **f32), torch.tensor(high, **f32)
        self.dt, self.integrate = float(dt), integrate_action
        self.alpha = None if action_lag is None else float(dt) / float(action_lag)
        self.sigma_a = None if action_noise is None else torch.tensor(action_noise, **f32)
        self.sigma_o = None if observation_noise is None else torch.tensor(observation_noise, **f32)
        self.prev_command = torch.zeros(num_envs, self.act_dim, **f32)
        self.command = torch.zeros(num_envs, self.act_dim, **f32)
        self.observation = torch.zeros(num_envs, self.stacked_dim, **f32)
        self.final_observation = torch.zeros(num_envs, self.stacked_dim, **f32)

    def state_tensors(self):
        return {"prev_command": self.prev_command, "observation": self.observation}

    def _frame(self, obs, command):
        import torch

        if self.sigma_o is not None:
            obs = obs + self.sigma_o * torch.randn_like(obs)
        return torch.cat([obs, command], dim=1)

    def reset(self, obs):
        self.observation.zero_()
        self.observation[:, -self.frame_dim:] = self._frame(obs, self.prev_command.zero_())
        return self.observation

    def shape_action(self, a):
        import torch

        p = self.prev_command
        u = torch.clamp(p + a * self.dt, self.low, self.high) if self.integrate else a
        if self.sigma_a is not None:
            u = torch.clamp(u + self.sigma_a * torch.randn_like(u), self.low, self.high)
        c = u if self.alpha is None else p + self.alpha * (u - p)
        self.command.copy_(c)
        self.prev_command.copy_(c)
        return self.command

    def observe(self, next_obs, terminated, truncated, final_obs=None):
        import torch

        F = self.frame_dim
        done = (terminated | truncated).unsqueeze(1)
        shifted = self.observation[:, F:]
        if final_obs is not None:
            torch.where(done, torch.cat([shifted, self._frame(final_obs, self.command)], dim=1), self.final_observation, out=self.final_observation)
        live = torch.cat([shifted, self._frame(next_obs, self.command)], dim=1)
        restart = torch.cat([torch.zeros_like(shifted), self._frame(next_obs, torch.zeros_like(self.command))], dim=1)
        torch.where(done, restart, live, out=self.observation)
        self.prev_command.masked_fill_(done, 0.0)
        return self.observation


class WideEnv:
    """The env with its observation (and final observation) widened to `words` columns by one strided copy each."""

    def __init__(self, env, words):
        import types

        import torch

        self.env, self.num_envs, self.device = env, env.num_envs, env.device
        self.single_observation_space = types.SimpleNamespace(shape=(words,))  # (what RunningNormalizer.for_env sizes itself by)
        self.observation = torch.zeros(env.num_envs, words, device=env.device)
        self.final = torch.zeros(env.num_envs, words, device=env.device)

    def reset(self, **kw):
        self.env.reset(**kw)
        self.observation[:, :D].copy_(self.env.observation)
        return self.observation, {}

    def step(self, action):
        obs, reward, terminated, truncated, info = self.env.step(action)
        self.observation[:, :D].copy_(obs)
        self.final[:, :D].copy_(info["final_obs"])
        return self.observation, reward, terminated, truncated, {"final_obs": self.final}


def _model(variant, noise=True):
    import torch
    import torch.nn as nn

    import upkie_amd.envs as envs
    from upkie_amd.pipeline import AgentPipeline
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.ppo import Ppo
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    env = envs.make("Upkie-HIP-Pendulum-Vec", num_envs=N, frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=400)
    dev = env.device
    kw = dict(stack=K, integrate_action=True, action_lag=LAG, action_noise=SIGMA_A if noise else None, observation_noise=SIGMA_O if noise else None)
    pipe = None
    if variant == "kernels":
        pipe = AgentPipeline(N, D, [-1.0], [1.0], DT, device=dev, **kw)
    elif variant == "torch":
        pipe = TorchPipeline(N, D, [-1.0], [1.0], DT, device=dev, **kw)
    words = D if variant == "none" else K * (D + A)
    tower = lambda: nn.Sequential(nn.Linear(words, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)  # noqa: E731
    policy = MlpActorCritic.from_modules(tower(), tower(), nn.Parameter(torch.zeros(1, device=dev)), action_low=[-2.0], action_high=[2.0])
    outer = WideEnv(env, words) if variant == "none40" else env
    model = Ppo(outer, policy, n_steps=T, batch_size=N * T // 4, pipeline=pipe,
                reward_fn=lambda obs, info: torch.abs(obs[:, 0]).neg_().add_(1.0))
    return env, model


def measure(variant, replays):
    import torch

    env, model = _model(variant)
    with env:
        model._setup()
        for _ in range(3):
            model._loop.replay()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(replays):
            model._loop.replay()
        end.record()
        torch.cuda.synchronize()
        us = start.elapsed_time(end) * 1e3 / (replays * T)
    print(json.dumps({"variant": variant, "us_per_rollout_step": round(us, 3), "num_envs": N, "stack": K, "obs_dim": D, "act_dim": A,
                      "n_steps": T, "replays": replays}), flush=True)


def check():
    """`TorchPipeline` against the kernels, noise off, integration and lag on, a tenth of the envs ending per step."""
    import torch

    from upkie_amd.pipeline import AgentPipeline

    dev, n = "cuda:0", 1000
    kw = dict(stack=K, integrate_action=True, action_lag=LAG)
    a, b = AgentPipeline(n, D, [-1.0], [1.0], DT, device=dev, **kw), TorchPipeline(n, D, [-1.0], [1.0], DT, device=dev, **kw)
    gen = torch.Generator(device=dev).manual_seed(0)
    first = torch.randn(n, D, device=dev, generator=gen)
    worst = 0.0
    moved = bool(torch.equal(a.reset(first)[:, -(D + A):-A], b.reset(first)[:, -(D + A):-A]))
    for _ in range(3 * K):
        act = torch.rand(n, A, device=dev, generator=gen) * 4 - 2
        nxt, fin = torch.randn(n, D, device=dev, generator=gen), torch.randn(n, D, device=dev, generator=gen)
        term, trunc = torch.rand(n, device=dev, generator=gen) < 0.05, torch.rand(n, device=dev, generator=gen) < 0.05
        worst = max(worst, float((a.shape_action(act) - b.shape_action(act)).abs().max()))
        b.prev_command.copy_(a.prev_command)  # (one step at a time: the composition continues from the kernels' command)
        b.command.copy_(a.command)
        oa, ob = a.observe(nxt, term, trunc, final_obs=fin), b.observe(nxt, term, trunc, final_obs=fin)
        done = term | trunc
        moved = moved and bool(torch.equal(oa, ob)) and bool(torch.equal(a.final_observation[done], b.final_observation[done]))
        moved = moved and bool(torch.equal(a.prev_command, b.prev_command))
    ok = moved and worst <= 4 * 2.0 ** -24
    print(json.dumps({"check": "TorchPipeline against the kernels, noise off", "stack_final_observation_and_restart_bit_equal": moved,
                      "worst_command_difference": worst, "bound": 4 * 2.0 ** -24, "ok": ok}), flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--variant", choices=VARIANTS, help="one measurement in this process (what the parent starts)")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--only-kernels", action="store_true", help="the kernels variant alone, for rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_agent_pipeline: no HIP device (there is no CPU fallback)")
    if args.check:
        sys.exit(0 if check() else 1)
    if args.variant or args.only_kernels:
        measure(args.variant or "kernels", args.replays)
        return
    results = {v: [] for v in VARIANTS}
    for _ in range(args.rounds):
        for v in VARIANTS:  # interleaved: a drift of the box shows in every variant alike
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", v, "--replays", str(args.replays)], capture_output=True,
                                 text=True, timeout=600)
            if out.returncode != 0:
                sys.exit(f"bench_agent_pipeline: variant {v} failed ({out.returncode}):\n{out.stderr[-2000:]}")
            results[v].append(json.loads(out.stdout.strip().splitlines()[-1])["us_per_rollout_step"])
    med = {v: statistics.median(x) for v, x in results.items()}
    for v in VARIANTS:
        print(json.dumps({"variant": v, "us_per_rollout_step_median": round(med[v], 3), "min": min(results[v]), "max": max(results[v]),
                          "rounds": results[v], "num_envs": N, "stack": K, "obs_dim": D, "act_dim": A, "n_steps": T}), flush=True)
    print(json.dumps({"what": "differences of the medians, us per rollout step", "kernels_minus_none": round(med["kernels"] - med["none"], 3),
                      "none40_minus_none": round(med["none40"] - med["none"], 3), "kernels_minus_none40": round(med["kernels"] - med["none40"], 3),
                      "torch_minus_kernels": round(med["torch"] - med["kernels"], 3)}), flush=True)


if __name__ == "__main__":
    main()
