"""ppo_learn_events.py under a push curriculum (`upkie_amd.events.PushLevels`): every env carries a difficulty level, decided
on the device in the events' own launch. An env starts at level 0, where its pushes are the weakest of the range; when its
episode reaches the time limit after at least one push, it goes up a level, and when the robot falls, down two. At level l
of 8 its push norms are uniform in 5 N to 5 + 25 * l / 8 N, so the batch is pushed as hard as each env's policy has shown
it can take, with no reduction over the batch and no decision on the host. An `EvalCallback` evaluates every other
iteration in an env of its own whose events sit at the top level (``PushLevels(8, start=8, up=0, down=0)``), the level
histogram is printed per iteration, and halfway through a callback doubles the push probability (`set_push`: a device
copy that the captured rollout follows at its next replay).
EXAMPLE_ENVS shortens the batch as EXAMPLE_STEPS shortens the rollout (smoke tests)."""
import os

import torch
import torch.nn as nn

from _common import steps

import upkie_amd.envs as envs
from upkie_amd.evaluation import EvalCallback
from upkie_amd.events import EpisodeEvents, PushLevels
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import Ppo
from upkie_amd.utils.robot_state import RobotState
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

LEVELS = 8
PUSHES = dict(push_prob=0.01, push_norm=(5.0, 30.0), push_steps=(10, 30))


def tower(d_in, d_out):  # SB3 MlpPolicy's default net_arch: [64, 64], tanh
    return nn.Sequential(nn.Linear(d_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, d_out))


def reward(obs, info):  # (a stand-in reward: the reference's is constant)
    return torch.abs(obs[:, 0]).neg_().add_(1.0)


if __name__ == "__main__":
    B, T, iterations = int(os.environ.get("EXAMPLE_ENVS", 4096)), steps(128), 4
    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    limit = min(200, max(T // 2, 2))  # (an episode has to be able to reach its time limit inside a short smoke run)
    kw = dict(frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=limit)
    make = lambda n, seed: envs.make("Upkie-HIP-Pendulum-Vec", num_envs=n, seed=seed, **kw)  # noqa: E731
    with make(B, 0) as env, make(min(B, 256), 1) as eval_env:
        events = EpisodeEvents(env, curriculum=PushLevels(LEVELS, start=0, up=1, down=2, min_pushes=1), live=True, **PUSHES)
        top = EpisodeEvents(eval_env, curriculum=PushLevels(LEVELS, start=LEVELS, up=0, down=0), **PUSHES)
        evaluate = EvalCallback(eval_env, n_eval_episodes=min(512, 4 * B), eval_freq=2 * T, reward_fn=reward, seed=2, events=top)
        actor, critic = tower(4, 1).to(env.device), tower(4, 1).to(env.device)
        policy = MlpActorCritic.from_modules(actor, critic, nn.Parameter(torch.zeros(1, device=env.device)), action_low=[-1.0], action_high=[1.0])
        model = Ppo(env, policy, n_steps=T, batch_size=B * T // 4, learning_rate=lambda p: 3e-4 * p, target_kl=0.03, reward_fn=reward, events=events)

        def callback(m, record):
            print(f"iteration {m.iterations}: envs per level {events.level_counts().tolist()}")
            if m.iterations == iterations // 2:
                events.set_push(prob=2.0 * PUSHES["push_prob"])
            return evaluate(m, record)

        model.learn(iterations * T * B, callback=callback)
        for record in model.records:
            print(f"record {record['time/iterations']}: " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in record.items()))
        print(f"training: {int(events.pushes.sum())} pushes started, {int(events.episodes.sum())} episodes ended in {int(events.calls[0])} steps of {B} "
              f"envs; evaluation at level {LEVELS}: {int(top.pushes.sum())} pushes, every env still at the top: {bool((top.level == LEVELS).all())}")
