"""Host cost of `Ppo`'s eager paths, the ones a process-group run takes (nothing is captured there): the host time to
issue one rollout step at 64 envs with ``graph=False``, without and with an `AgentPipeline`, and to issue one eager
`PpoTrainer.update` of 2 epochs x 4 minibatches. ``time.perf_counter`` around `collect_rollouts()` / `update()`, the
device synchronised after the clock is read. One JSON line.

``--package-root DIR`` imports `upkie_amd` from another checkout (the parent commit's, with ``UPKIE_HIP_LIBRARY``
pointing at this tree's library) so that two versions of the Python side alternate on one GPU:

    python tools/bench_ppo_host.py [--package-root DIR] [--reps 30]"""

import argparse
import json
import os
import statistics
import sys
import time

N, T, D, A, K = 64, 128, 4, 1, 2


def _model(pipeline):
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
    pipe = AgentPipeline(N, D, [-1.0], [1.0], 1.0 / 200.0, stack=K, integrate_action=True, device=dev) if pipeline else None
    words = K * (D + A) if pipeline else D
    tower = lambda: nn.Sequential(nn.Linear(words, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)  # noqa: E731
    policy = MlpActorCritic.from_modules(tower(), tower(), nn.Parameter(torch.zeros(1, device=dev)), action_low=[-1.0], action_high=[1.0])
    model = Ppo(env, policy, n_steps=T, n_epochs=2, batch_size=N * T // 4, pipeline=pipe, graph=False,
                reward_fn=lambda obs, info: torch.abs(obs[:, 0]).neg_().add_(1.0))
    return env, model


def _host_us(call, reps, per):
    import torch

    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        begin = time.perf_counter()
        call()
        times.append((time.perf_counter() - begin) * 1e6 / per)
        torch.cuda.synchronize()
    return round(statistics.median(times), 3)


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--package-root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    parser.add_argument("--reps", type=int, default=30)
    args = parser.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    result = {"package_root": os.path.abspath(args.package_root), "num_envs": N, "n_steps": T, "reps": args.reps}
    for name, pipeline in (("rollout_step_us", False), ("rollout_step_pipeline_us", True)):
        env, model = _model(pipeline)
        with env:
            model._setup()
            model.collect_rollouts()  # (warm-up)
            result[name] = _host_us(model.collect_rollouts, args.reps, T)
            if not pipeline:
                model.trainer.prepare(model.buffer)
                model.trainer.update(model.buffer)  # (warm-up)
                result["update_2x4_us"] = _host_us(lambda: model.trainer.update(model.buffer), args.reps, 1)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
