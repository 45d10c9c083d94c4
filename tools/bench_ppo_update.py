"""The PPO update (upkie_amd.ppo.PpoTrainer, csrc/ppo.hpp) against the same SB3 minibatch as torch ops, at obs 4,
[64, 64] tanh towers, act 1 (and [256, 256] at the large size): one minibatch update (advantage statistics + gradient,
fold, Adam) event-timed, eager and replayed from a hipGraph; the torch minibatch (gather, advantage normalisation,
Normal, clipped surrogate, autograd, clip_grad_norm_, Adam) eager and graphed (capturable Adam); one whole PPO iteration
(128-step graphed rollout of 4096 envs + 10 epochs x 4 minibatches) with each learner. One JSON line per measurement.
Kernel times: run under ``rocprofv3 --kernel-trace --stats -- python tools/bench_ppo_update.py --only-kernels``."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from upkie_amd.policies import MlpActorCritic  # noqa: E402
from upkie_amd.ppo import PpoTrainer  # noqa: E402
from upkie_amd.rollout import RolloutBuffer  # noqa: E402

DEV = "cuda:0"


def tower(d_in, width, d_out):
    return nn.Sequential(nn.Linear(d_in, width), nn.Tanh(), nn.Linear(width, width), nn.Tanh(), nn.Linear(width, d_out)).to(DEV)


def setup(T, N, width):
    torch.manual_seed(0)
    actor, critic = tower(4, width, 1), tower(4, width, 1)
    log_std = nn.Parameter(torch.zeros(1, device=DEV))
    pol = MlpActorCritic.from_modules(actor, critic, log_std, [-1.0], [1.0], seed=0)
    buf = RolloutBuffer(T, N, obs_shape=(4,), action_shape=(1,), device=DEV)
    g = torch.Generator(DEV).manual_seed(1)
    buf.observations.copy_(torch.randn(T, N, 4, device=DEV, generator=g))
    for t in range(T):
        pol.act(buf.observations[t], out={"action": buf.actions[t], "value": buf.values[t], "log_prob": buf.log_probs[t]})
    buf.log_probs.add_(0.1 * torch.randn(T, N, device=DEV, generator=g))
    buf.advantages = torch.randn(T, N, device=DEV, generator=g)
    buf.returns = (buf.values + torch.randn(T, N, device=DEV, generator=g)).contiguous()
    buf.pos, buf.full = T, True
    return pol, actor, critic, log_std, buf


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return {"median_us": times[len(times) // 2], "min_us": times[0]}


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def torch_learner(actor, critic, log_std, buf, batch, capturable):
    """One SB3 minibatch as torch ops over `idx` (a persistent index buffer the caller fills)."""
    params = [log_std] + list(actor.parameters()) + list(critic.parameters())
    opt = torch.optim.Adam(params, lr=3e-4, eps=1e-5, capturable=capturable)
    total = buf.buffer_size * buf.n_envs
    flat = [buf.observations.reshape(total, -1), buf.actions.reshape(total, -1), buf.values.reshape(total), buf.log_probs.reshape(total),
            buf.advantages.reshape(total), buf.returns.reshape(total)]
    idx = torch.randperm(total, device=DEV)[:batch]

    def step():
        obs, act, _, old_lp, adv, ret = (t[idx] for t in flat)
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        mean = actor(obs)
        dist = torch.distributions.Normal(mean, torch.ones_like(mean) * log_std.exp(), validate_args=False)  # (the check syncs)
        ratio = torch.exp(dist.log_prob(act).sum(1) - old_lp)
        pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 0.8, 1.2)).mean()
        vl = nn.functional.mse_loss(ret, critic(obs).flatten())
        ent = -torch.mean(dist.entropy().sum(1))
        loss = pl + 0.0 * ent + 0.5 * vl
        opt.zero_grad(set_to_none=False)
        loss.backward()
        nn.utils.clip_grad_norm_(params, 0.5)
        opt.step()

    return step, idx


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def minibatch_rows(samples, width, reps, out, with_torch=True):
    T = 128 if samples >= 128 * 16 else 1
    pol, actor, critic, log_std, buf = setup(T, samples // T, width)
    tr = PpoTrainer(pol, n_epochs=1, batch_size=samples)
    tr.train(buf, sync=False)
    fn = lambda: tr.update(buf, sync=False)  # noqa: E731  (advantage stats + gradient + fold + Adam)
    base = {"samples": samples, "towers": [width, width]}
    emit(dict(base, learner="hip", mode="eager", launches=4, **timed(fn, reps)), out)
    emit(dict(base, learner="hip", mode="graph", launches=4, **timed(graphed(fn), reps)), out)
    if with_torch:
        step, _ = torch_learner(actor, critic, log_std, buf, samples, capturable=False)
        emit(dict(base, learner="torch", mode="eager", **timed(step, reps)), out)
        step, _ = torch_learner(actor, critic, log_std, buf, samples, capturable=True)
        emit(dict(base, learner="torch", mode="graph", **timed(graphed(step), reps)), out)


def iteration_rows(reps, out):
    """128-step graphed rollout of 4096 envs + 10 epochs x 4 minibatches of 131072 samples."""
    import upkie_amd.envs as envs
    from upkie_amd.graphs import GraphedLoop

    B, T = 4096, 128
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=B, frequency=200.0, autoreset_mode="same_step", max_episode_steps=400) as env:
        pol, actor, critic, log_std, buf = setup(T, B, 64)
        env.reset(seed=0)
        obs = env.observation
        starts = torch.ones(B, dtype=torch.uint8, device=DEV)
        slot = {"t": T - 1}

        def rollout_step():
            t = slot["t"]
            buf.episode_starts[t].copy_(starts)
            o = pol.act(obs, out={"norm_obs": buf.observations[t], "action": buf.actions[t], "value": buf.values[t], "log_prob": buf.log_probs[t]})
            _, reward, term, trunc, _ = env.step(o[0])
            buf.rewards[t].copy_(reward)
            torch.logical_or(term, trunc, out=starts)
            slot["t"] = (t + 1) % T

        loop = GraphedLoop(rollout_step, unroll=T, warmup=1)
        last = torch.zeros(B, device=DEV)

        def gae():
            buf.compute_returns_and_advantage(last_values=last, dones=starts)

        loop.replay()
        gae()
        tr = PpoTrainer(pol, n_epochs=10, batch_size=B * T // 4)
        tr.train(buf, sync=False)
        emit({"what": "rollout_128_steps", **timed(loop.replay, reps)}, out)
        emit({"what": "ppo_iteration", "learner": "hip", **timed(lambda: (loop.replay(), gae(), tr.train(buf, sync=False)), reps)}, out)
        for capturable in (False, True):
            step, idx = torch_learner(actor, critic, log_std, buf, B * T // 4, capturable)
            run = graphed(step) if capturable else step
            total = B * T
            gen = torch.Generator(DEV).manual_seed(0)

            def learner():
                for _ in range(10):
                    perm = torch.randperm(total, device=DEV, generator=gen)
                    for j in range(4):
                        idx.copy_(perm[j * (total // 4):(j + 1) * (total // 4)])
                        run()

            emit({"what": "ppo_iteration", "learner": "torch", "mode": "graph" if capturable else "eager",
                  **timed(lambda: (loop.replay(), gae(), learner()), max(3, reps // 4), warmup=1)}, out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--only-kernels", action="store_true", help="only the HIP minibatch updates (for rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    with_torch = not args.only_kernels
    minibatch_rows(131072, 64, args.reps, args.out, with_torch)
    minibatch_rows(4096, 64, args.reps, args.out, with_torch)
    minibatch_rows(131072, 256, max(5, args.reps // 5), args.out, with_torch)
    if with_torch:
        iteration_rows(max(5, args.reps // 5), args.out)


if __name__ == "__main__":
    main()
