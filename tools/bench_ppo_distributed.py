"""Cost of the data-parallel form (PpoTrainer / RunningNormalizer with a process group) on a one-rank RCCL group, where
it computes the same bits as the fused form: one minibatch update (advantage statistics + gradient, fold, Adam) at
obs 4, [64, 64] tanh towers, act 1, fused vs split around the exchanges, and one normaliser step (moments, merge, apply)
at 4096 envs x 4 words with and without the group. Event-timed on the stream, host overhead of the collectives
included; one JSON line per measurement. Run it as

    UPKIE_FORCE_PROCESS_GROUP=1 python -m torch.distributed.run --nproc-per-node 1 tools/bench_ppo_distributed.py

One GPU cannot show multi-rank scaling: these numbers are the fixed cost the split adds, not what W ranks gain."""
import argparse
import json
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_ppo_update import setup, timed  # noqa: E402
from upkie_amd.distributed import init_distributed  # noqa: E402
from upkie_amd.normalize import RunningNormalizer  # noqa: E402
from upkie_amd.ppo import PpoTrainer  # noqa: E402

DEV = "cuda:0"


def bench_update(group, T, N, reps):
    pol, _, _, _, buf = setup(T, N, 64)
    rows = {}
    for form, g in (("fused", None), ("split", group)):
        tr = PpoTrainer(pol, n_epochs=1, batch_size=T * N, seed=0, process_group=g)
        tr.prepare(buf)
        rows[form] = timed(lambda: tr.update(buf, sync=False), reps)
        print(json.dumps({"what": f"one minibatch update ({form}: " + ("advantage stats + gradient, fold, Adam)" if g is None else
                          "advantage partials x2 + finish, gradient + local fold, exchange, fold over slots, Adam; 3 exchanges)"),
                          "samples": T * N, "widths": [64, 64], "world": 1 if g is None else dist.get_world_size(g), **rows[form]}), flush=True)
    print(json.dumps({"what": "added by the split (median)", "samples": T * N, "us": rows["split"]["median_us"] - rows["fused"]["median_us"]}), flush=True)


def bench_normalizer(group, N, D, reps):
    gen = torch.Generator(DEV).manual_seed(0)
    obs = torch.randn(N, D, device=DEV, generator=gen)
    reward = torch.randn(N, device=DEV, generator=gen)
    term = torch.zeros(N, dtype=torch.uint8, device=DEV)
    out = {"norm_obs": torch.empty(N, D, device=DEV), "reward": torch.empty(N, device=DEV), "episode_starts": torch.empty_like(term)}
    rows = {}
    for form, g in (("no group", None), ("group", group)):
        norm = RunningNormalizer(N, D, device=DEV, process_group=g)
        norm.reset(obs)
        rows[form] = timed(lambda: norm.step(obs, reward, term, out=out), reps)
        print(json.dumps({"what": f"normaliser step, {form} (" + ("moments + apply)" if g is None else "local moments, exchange, merge + apply)"),
                          "num_envs": N, "obs_dim": D, **rows[form]}), flush=True)
    print(json.dumps({"what": "added by the group (median)", "num_envs": N, "us": rows["group"]["median_us"] - rows["no group"]["median_us"]}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    init_distributed()
    if not dist.is_initialized():
        raise SystemExit("run under torch.distributed.run with UPKIE_FORCE_PROCESS_GROUP=1 (a one-rank RCCL group)")
    group = dist.group.WORLD
    print(json.dumps({"device": torch.cuda.get_device_name(0), "backend": dist.get_backend(group), "world": dist.get_world_size(group)}), flush=True)
    for T, N in ((32, 4096), (1, 4096)):
        bench_update(group, T, N, args.reps)
    bench_normalizer(group, 4096, 4, 4 * args.reps)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
