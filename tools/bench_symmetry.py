"""What mirror symmetry (`PpoTrainer(symmetry=)`, `upkie_ppo_minibatch_update_mirror`) costs in the PPO update: one process,
131072 samples, [64, 64] tanh towers on the Gyropod shape with two targets (D = 8, A = 2). Device events around
back-to-back hipGraph replays of 10 updates, `--repeats` samples each, the sides in alternating rounds in one process (as
tools/bench_distillation.py), one JSON line with the medians and ranges:

  us_mirror     the mirrored update of B samples with `augment` on: 2 B positions through the towers;
  us_plain      the plain update of the same B samples;
  us_plain_2b   the plain update of 2 B samples: the yardstick -- the same number of tiles through the same towers;
  ratio         us_mirror / us_plain_2b (expected near 1: the extras per pair are the table gathers and one pass of A words
                through the stage), ratio_plain = us_mirror / us_plain.

Every update includes its advantage-statistics launch, as a trainer issues it (over B samples on the mirrored side, over
2 B on the yardstick's). lr 0: the weights stay where they are. `--variant NAME` (mirror, plain, plain_2b) runs one side
alone: the program to put behind ``rocprofv3 --kernel-trace --stats --``.

usage: python tools/bench_symmetry.py [--samples 131072] [--repeats 5] [--iters 100] [--variant NAME]
                                      [--out profiles/symmetry_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, A = 8, 2


def _sample(fn, iters):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def _side(n, symmetry):
    """A graph of 10 updates of one minibatch of n samples (and what it reads, kept alive)."""
    import torch
    import torch.nn as nn

    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.ppo import PpoTrainer
    from upkie_amd.rollout import RolloutBuffer

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tower = lambda d_out: nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, d_out)).to(dev)  # noqa: E731
    policy = MlpActorCritic.from_modules(tower(A), tower(1), nn.Parameter(torch.zeros(A, device=dev)), action_low=[-2.0, -1.0],
                                         action_high=[2.0, 1.0], seed=0)
    buf = RolloutBuffer(1, n, obs_shape=(D,), action_shape=(A,), device=dev)
    buf.observations.copy_(torch.randn(1, n, D, device=dev))
    policy.act(buf.observations[0], out={"action": buf.actions[0], "value": buf.values[0], "log_prob": buf.log_probs[0]})
    buf.advantages, buf.returns = torch.randn(1, n, device=dev), torch.randn(1, n, device=dev)
    buf.pos, buf.full = 1, True
    trainer = PpoTrainer(policy, lr=0.0, n_epochs=1, batch_size=n, symmetry=symmetry)
    trainer.prepare(buf)
    trainer.update(buf, sync=False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(10):
            trainer.update(buf, sync=False)
    return graph, (trainer, buf, policy)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--samples", type=int, default=131072)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--iters", type=int, default=100)
    parser.add_argument("--variant", choices=("mirror", "plain", "plain_2b"))
    parser.add_argument("--label", default="")
    parser.add_argument("--out")
    args = parser.parse_args()
    import torch

    from upkie_amd.symmetry import MirrorSymmetry

    B = args.samples
    symmetry = MirrorSymmetry.gyropod(("ground_velocity", "yaw_velocity"), augment=True, mirror_coef=0.5)
    build = {"mirror": lambda: _side(B, symmetry), "plain": lambda: _side(B, None), "plain_2b": lambda: _side(2 * B, None)}
    names = [args.variant] if args.variant else list(build)
    sides = {name: build[name]() for name in names}
    iters = max(1, args.iters // 10)
    for graph, _ in sides.values():
        for _ in range(3):
            graph.replay()
    torch.cuda.synchronize()
    samples = {name: [] for name in names}
    for _ in range(args.repeats):
        for name in names:  # (alternating: a drift of the clocks reaches every side alike)
            samples[name].append(_sample(sides[name][0].replay, iters) / 10)
    out = {"bench": "symmetry", "label": args.label, "samples": B, "obs_dim": D, "act_dim": A, "towers": [64, 64], "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0)}
    for name, s in samples.items():
        out.update({f"us_{name}_median": round(statistics.median(s), 3), f"us_{name}_min": round(min(s), 3), f"us_{name}_max": round(max(s), 3)})
    if not args.variant:
        out["ratio"] = round(out["us_mirror_median"] / out["us_plain_2b_median"], 4)
        out["ratio_plain"] = round(out["us_mirror_median"] / out["us_plain_median"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
