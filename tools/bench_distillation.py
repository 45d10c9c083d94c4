"""What policy distillation (`upkie_amd.distill`) costs at 4096 envs and [64, 64] towers (`--num-envs N`: at N). Device
events around back-to-back hipGraph replays, `--repeats` samples each; one JSON line per variant with the median and the
range (min, max) over the samples. The two sides of every comparison are timed in the same process in alternating rounds,
as tools/bench_ppo_learn.py does, so that a drift of the clocks reaches both alike.

  update_131072, update_4096   one minibatch update (gradient launch, fold, Adam) of that many samples, pendulum shape
                               (D = 4, A = 1), replayed from a graph of 10: `us_distill` the behaviour-cloning update,
                               `us_ppo` the PPO update of the same shape and minibatch, `ratio` = distill / ppo. The
                               gradient launch alone is not an entry point; `us_*_floor` is the same update on ONE sample
                               (the fold, Adam and a one-tile gradient launch), so `us_*_gradient` = update - floor is what
                               the samples cost in the gradient launch;
  mix_1, mix_64                the mix launch alone at act_dim 1 and 64, eager and graphed (`us_graphed_*`);
  rollout                      one graphed rollout step on the pendulum env behind an `AgentPipeline` of 8 frames:
                               `us_per_step_ppo` (`Ppo`: actor and critic), `us_per_step_distill` (`Distillation` with an
                               `MlpActorCritic` teacher on the raw observation), `us_per_step_no_teacher` (the same with a
                               teacher that launches nothing: the label is a constant), and the differences.

`--variant NAME` runs one of these alone: the program to put behind ``rocprofv3 --kernel-trace --stats --``, whose kernel
statistics give the gradient launch's own time (`ppo_grad_kernel<W, ACT, true>` is the behaviour-cloning launch,
`<W, ACT, false>` PPO's), where `us_*_gradient` above is an estimate (an update less its one-sample floor).

usage: python tools/bench_distillation.py [--label NAME] [--repeats 5] [--iters 200] [--num-envs 4096] [--variant NAME]
                                          [--out profiles/distillation_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, iters, repeats):
    """Microseconds per call of `fn`: `repeats` samples of `iters` calls between two device events."""
    import torch

    for _ in range(3):
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


def _figures(samples, key="us"):
    return {f"{key}_median": round(statistics.median(samples), 3), f"{key}_min": round(min(samples), 3), f"{key}_max": round(max(samples), 3)}


def _alternate(sides, iters, repeats):
    """{name: samples} of several callables, one sample of each per round."""
    out = {name: [] for name in sides}
    for _ in range(repeats):
        for name, fn in sides.items():
            out[name] += _time(fn, iters, 1)
    return out


def _tower(d_in, d_out, dev, width=64):
    import torch.nn as nn

    return nn.Sequential(nn.Linear(d_in, width), nn.Tanh(), nn.Linear(width, width), nn.Tanh(), nn.Linear(width, d_out)).to(dev)


def _policy(d_in, dev, seed=0):
    import torch
    import torch.nn as nn

    from upkie_amd.policies import MlpActorCritic

    torch.manual_seed(seed)
    return MlpActorCritic.from_modules(_tower(d_in, 1, dev), _tower(d_in, 1, dev), nn.Parameter(torch.zeros(1, device=dev)), action_low=[-1.0],
                                       action_high=[1.0], seed=seed)


def _graph_of(fn, count=10):
    import torch

    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(count):
            fn()
    return graph


def update(samples, iters, repeats):
    """One minibatch of `samples` rows, and of one row, under both updates (lr 0: the weights stay where they are)."""
    import torch

    from upkie_amd.distill import DistillTrainer
    from upkie_amd.ppo import PpoTrainer
    from upkie_amd.rollout import RolloutBuffer

    dev = torch.device("cuda:0")
    sides = {}
    for n in (samples, 1):
        key = "" if n == samples else "_floor"
        student = _policy(4, dev, seed=1)
        obs, labels = torch.randn(1, n, 4, device=dev), torch.randn(1, n, 1, device=dev)
        bc = DistillTrainer(student, lr=0.0, n_epochs=1, batch_size=n)
        bc.prepare(obs, labels)
        graph_bc = _graph_of(lambda: bc.update(obs, labels, sync=False))
        policy = _policy(4, dev, seed=2)
        buf = RolloutBuffer(1, n, obs_shape=(4,), action_shape=(1,), device=dev)
        buf.observations.copy_(obs)
        policy.act(buf.observations[0], out={"action": buf.actions[0], "value": buf.values[0], "log_prob": buf.log_probs[0]})
        buf.advantages, buf.returns = torch.randn(1, n, device=dev), torch.randn(1, n, device=dev)
        buf.pos, buf.full = 1, True
        ppo = PpoTrainer(policy, lr=0.0, n_epochs=1, batch_size=n)
        ppo.prepare(buf)
        graph_ppo = _graph_of(lambda: ppo.update(buf, sync=False))
        sides["us_distill" + key], sides["us_ppo" + key] = graph_bc.replay, graph_ppo.replay
        sides["_keep" + key] = (bc, ppo, buf, obs, labels, graph_bc, graph_ppo)
    keep = {k: v for k, v in sides.items() if k.startswith("_keep")}
    timed = _alternate({k: v for k, v in sides.items() if not k.startswith("_keep")}, max(1, iters // 10), repeats)
    out = {}
    for name, s in timed.items():
        out.update(_figures([us / 10 for us in s], name))  # (a graph holds 10 updates; PPO's also its advantage statistics launch)
    for side in ("distill", "ppo"):
        out[f"us_{side}_gradient"] = round(out[f"us_{side}_median"] - out[f"us_{side}_floor_median"], 3)
    out["ratio"] = round(out["us_distill_median"] / out["us_ppo_median"], 4)
    out["ratio_gradient"] = round(out["us_distill_gradient"] / out["us_ppo_gradient"], 4) if out["us_ppo_gradient"] > 0 else None
    del keep
    return out


def mix(n, act_dim, iters, repeats):
    import torch

    from upkie_amd import abi
    from upkie_amd.distill import DaggerMix
    from upkie_amd.graphs import GraphedLoop
    from upkie_amd.model.default_model import default_model
    from upkie_amd.sim import BatchedSim

    sim = BatchedSim(abi.default_sim_config(n, seed=0), default_model())
    stage = DaggerMix(sim, act_dim, [-1.0] * act_dim, [1.0] * act_dim, beta=0.5)
    label, action = torch.randn(n, act_dim, device=sim.device), torch.randn(n, act_dim, device=sim.device)
    fn = lambda: stage.step(label, action)  # noqa: E731
    eager = _time(fn, iters, repeats)
    loop = GraphedLoop(fn, unroll=100, warmup=1, device=sim.device)
    graphed = [us / 100 for us in _time(loop.replay, max(1, iters // 20), repeats)]
    sim.close()
    return dict(_figures(eager), **_figures(graphed, "us_graphed"), act_dim=act_dim)


class _ConstantTeacher:
    """A teacher that launches nothing: the label buffers keep their zeros."""

    obs_dim, act_dim = 4, 1

    def __call__(self, obs, out):
        return out


def _env(n, seed):
    import upkie_amd.envs as envs
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    return envs.make("Upkie-HIP-Pendulum-Vec", num_envs=n, frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=400, seed=seed)


def rollout(n, iters, repeats, steps=32):
    from upkie_amd.distill import Distillation
    from upkie_amd.pipeline import AgentPipeline
    from upkie_amd.ppo import Ppo

    def pipeline(dev):
        return AgentPipeline(n, 4, [-1.0], [1.0], dt=1.0 / 200.0, stack=8, action_lag=0.05, observation_noise=[0.002, 0.002, 0.01, 0.01], seed=0, device=dev)

    env_a, env_b, env_c = _env(n, 0), _env(n, 1), _env(n, 2)
    with env_a, env_b, env_c:
        dev = env_a.device
        pipes = [pipeline(dev) for _ in range(3)]
        ppo = Ppo(env_a, _policy(pipes[0].stacked_dim, dev), n_steps=steps, batch_size=n * steps // 4, pipeline=pipes[0])
        taught = Distillation(env_b, _policy(pipes[1].stacked_dim, dev, 1), _policy(4, dev, 2), n_steps=steps, batch_size=n * steps // 4, beta=0.5,
                              pipeline=pipes[1])
        free = Distillation(env_c, _policy(pipes[2].stacked_dim, dev, 3), _ConstantTeacher(), n_steps=steps, batch_size=n * steps // 4, beta=0.5,
                            pipeline=pipes[2])
        for model in (ppo, taught, free):
            model._setup()  # (captures the rollout: `steps` steps per replay)
        timed = _alternate({"us_per_step_ppo": ppo._loop.replay, "us_per_step_distill": taught._loop.replay, "us_per_step_no_teacher": free._loop.replay},
                           max(1, iters // 20), repeats)
        out = {}
        for name, s in timed.items():
            out.update(_figures([us / steps for us in s], name))
        out["us_teacher"] = round(out["us_per_step_distill_median"] - out["us_per_step_no_teacher_median"], 3)
        out["us_distill_minus_ppo"] = round(out["us_per_step_distill_median"] - out["us_per_step_ppo_median"], 3)
        return out


VARIANTS = ("update_131072", "update_4096", "mix_1", "mix_64", "rollout")


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--label", default="this tree")
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--iters", type=int, default=200)
    parser.add_argument("--num-envs", type=int, default=4096)
    parser.add_argument("--out", help="append the result lines to this file")
    parser.add_argument("--variant", choices=VARIANTS, help="run this variant alone (for rocprofv3 --kernel-trace --stats)")
    args = parser.parse_args()
    n, it, rep = args.num_envs, args.iters, args.repeats
    variants = [("update_131072", lambda: update(131072, it, rep)), ("update_4096", lambda: update(4096, it, rep)), ("mix_1", lambda: mix(n, 1, it, rep)),
                ("mix_64", lambda: mix(n, 64, it, rep)), ("rollout", lambda: rollout(n, it, rep))]
    assert [name for name, _ in variants] == list(VARIANTS)
    if args.variant:
        variants = [(name, run) for name, run in variants if name == args.variant]
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
