"""What the privileged critic (an asymmetric `MlpActorCritic`, `upkie_amd.privileged.PrivilegedObservation`,
`Ppo(critic_observation=...)`) costs at 4096 envs (`--num-envs N`: at N) with [64, 64] towers, and that the symmetric
launches did not get slower. Device events around `--iters` back-to-back launches, `--repeats` samples each; one JSON
line per variant with the median and the range (min, max) over the samples:

  policy_sym      `policy.act` (sampling, every output), symmetric, D = 40;
  policy_asym     the same launch with a critic row of its own, D = 40, Dc = 24;
  stage           the privileged stage's launch (4 observation words, 1 command, 3 force, 12 link scales: Dc = 20);
  update_sym      one minibatch of T N = 32 x N samples (131072 at 4096 envs) of the PPO update (gradient launch, fold,
                  Adam), symmetric, D = 40;
  update_asym     the same with Dc = 24: the restage adds one x load per sample per chunk;
  rollout         one graphed `Ppo` rollout step on the pendulum env with an `AgentPipeline` (8 frames: D = 40) and
                  `EpisodeEvents`, without and with `critic_observation=` (Dc = 20), two `Ppo` objects whose replays
                  alternate: `us_per_step`, `us_per_step_privileged`, `us_privileged` the difference.

`--tree DIR` imports the package from another checkout of the project that has been built (the parent commit, for the
yardstick): a tree without the feature runs the symmetric variants only. Run the parent and this tree in one session;
the parent's range over its five repeats is the session's run-to-run spread that the symmetric numbers are held to.

usage: python tools/bench_privileged_critic.py [--tree DIR] [--label NAME] [--repeats 5] [--iters 200] [--num-envs 4096]
                                               [--out profiles/privileged_critic_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, DC, T = 40, 24, 32


def _time(fn, iters, repeats):
    """Microseconds per call of `fn`: `repeats` samples of `iters` calls between two device events."""
    import torch

    for _ in range(10):
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


def _tower(d_in, dev):
    import torch.nn as nn

    return nn.Sequential(nn.Linear(d_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)


def _policy(dc, dev="cuda:0"):
    import torch
    import torch.nn as nn

    from upkie_amd.policies import MlpActorCritic

    torch.manual_seed(0)
    mean, var = torch.zeros(D), torch.ones(D)
    kw = dict(critic_obs_mean=torch.zeros(dc), critic_obs_var=torch.ones(dc)) if dc else {}
    return MlpActorCritic.from_modules(_tower(D, dev), _tower(dc or D, dev), nn.Parameter(torch.zeros(1, device=dev)), action_low=[-1.0],
                                       action_high=[1.0], obs_mean=mean, obs_var=var, **kw)


def policy_launch(dc, n, iters, repeats):
    import torch

    pol = _policy(dc)
    obs = torch.randn(n, D, device="cuda:0")
    kw = dict(critic_obs=torch.randn(n, dc, device="cuda:0")) if dc else {}
    return _figures(_time(lambda: pol.act(obs, **kw), iters, repeats))


def update_launch(dc, n, iters, repeats):
    import ctypes as C

    import torch

    from upkie_amd.launch import ptr
    from upkie_amd.ppo import PpoTrainer
    from upkie_amd.rollout import RolloutBuffer

    pol = _policy(dc)
    total = T * n
    kw = dict(critic_obs_shape=(dc,)) if dc else {}
    buf = RolloutBuffer(T, n, obs_shape=(D,), action_shape=(1,), device="cuda:0", **kw)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    for t in (buf.observations, buf.actions, buf.values, buf.log_probs) + ((buf.critic_observations,) if dc else ()):
        t.copy_(torch.randn(t.shape, generator=g, device="cuda:0") * 0.3)
    buf.advantages, buf.returns = torch.randn(T, n, generator=g, device="cuda:0"), torch.randn(T, n, generator=g, device="cuda:0")
    buf.pos, buf.full = T, True
    tr = PpoTrainer(pol, n_epochs=1, batch_size=total, lr=0.0, seed=0)  # (lr 0: every sample times the same weights)
    tr.prepare(buf)
    head = (C.byref(pol.shape), C.byref(tr.config))
    tensors = (buf.observations,) + ((buf.critic_observations,) if dc else ()) + (buf.actions, buf.values, buf.log_probs, tr.advantages, tr.returns)
    data = tuple(ptr(t) for t in tensors)
    perm = ptr(tr.perm[0])
    tr._advantage_stats(0, total, perm, data[-2])
    return dict(_figures(_time(lambda: tr._minibatch(0, 0, head, total, 0, total, perm, data), max(1, iters // 10), repeats)), samples=total)


def stage_launch(n, iters, repeats):
    import torch

    from upkie_amd.privileged import PrivilegedObservation

    dev = torch.device("cuda:0")
    env = types.SimpleNamespace(num_envs=n, device=dev, model=types.SimpleNamespace(num_links=13, link_randomized=[0] + [1] * 12))
    events = types.SimpleNamespace(num_envs=n, force=torch.randn(1, 3, n, device=dev), link_scale=torch.rand(24, n, device=dev) + 0.5)
    pipeline = types.SimpleNamespace(num_envs=n, obs_dim=4, act_dim=1, command=torch.randn(n, 1, device=dev))
    stage = PrivilegedObservation(env, events=events, pipeline=pipeline)
    obs, final = torch.randn(n, 4, device=dev), torch.randn(n, 4, device=dev)
    done = (torch.rand(n, device=dev) < 0.005).to(torch.uint8)
    stage.reset(obs)
    return dict(_figures(_time(lambda: stage.step(obs, done, None, final_obs=final), iters, repeats)), row_words=stage.dim)


def _reward(obs, info):
    import torch

    return torch.abs(obs[:, 0]).neg_().add_(1.0)


def _ppo(n, privileged):
    import torch
    import torch.nn as nn

    import upkie_amd.envs as envs
    from upkie_amd.events import EpisodeEvents
    from upkie_amd.pipeline import AgentPipeline
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.ppo import Ppo
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    env = envs.make("Upkie-HIP-Pendulum-Vec", num_envs=n, frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=400)
    dev = env.device
    events = EpisodeEvents(env, push_prob=0.01, push_norm=(5.0, 20.0), push_steps=(10, 30), inertia_variation=0.2)
    pipeline = AgentPipeline(n, 4, [-1.0], [1.0], dt=1.0 / 200.0, stack=8, observation_noise=[0.01] * 4, device=dev)
    kw, dc = {}, D
    if privileged:
        from upkie_amd.privileged import PrivilegedObservation

        kw["critic_observation"] = PrivilegedObservation(env, events=events, pipeline=pipeline)
        dc = kw["critic_observation"].dim
    policy = MlpActorCritic.from_modules(_tower(D, dev), _tower(dc, dev), nn.Parameter(torch.zeros(1, device=dev)), action_low=[-1.0], action_high=[1.0])
    model = Ppo(env, policy, n_steps=128, batch_size=n * 128 // 4, reward_fn=_reward, events=events, pipeline=pipeline, **kw)
    model._setup()  # (captures the rollout: 128 steps per replay)
    return env, model


def rollout(n, iters, repeats, feature):
    env_a, plain = _ppo(n, False)
    replays = max(1, iters // 40)
    if not feature:
        with env_a:
            return _figures([us / 128 for us in _time(plain._loop.replay, replays, repeats)], "us_per_step")
    env_b, priv = _ppo(n, True)
    with env_a, env_b:
        a, b = [], []
        for _ in range(repeats):  # alternate, so that a drift of the clocks reaches both alike
            a += [us / 128 for us in _time(plain._loop.replay, replays, 1)]
            b += [us / 128 for us in _time(priv._loop.replay, replays, 1)]
        out = dict(_figures(a, "us_per_step"), **_figures(b, "us_per_step_privileged"))
        out["us_privileged"] = round(out["us_per_step_privileged_median"] - out["us_per_step_median"], 3)
        return out


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--tree", default=ROOT, help="the checkout whose package is measured (default: this one)")
    parser.add_argument("--label", default="this tree")
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--iters", type=int, default=200)
    parser.add_argument("--num-envs", type=int, default=4096)
    parser.add_argument("--out", help="append the result lines to this file")
    args = parser.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from upkie_amd import policies

    feature = hasattr(policies, "asymmetric_shape")
    n, it, rep = args.num_envs, args.iters, args.repeats
    variants = [("policy_sym", lambda: policy_launch(0, n, it, rep)), ("update_sym", lambda: update_launch(0, n, it, rep))]
    if feature:
        variants += [("policy_asym", lambda: policy_launch(DC, n, it, rep)), ("update_asym", lambda: update_launch(DC, n, it, rep)),
                     ("stage", lambda: stage_launch(n, it, rep))]
    variants.append(("rollout", lambda: rollout(n, it, rep, feature)))
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
