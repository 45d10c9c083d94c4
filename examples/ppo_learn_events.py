"""ppo_learn.py under the perturbations a balancing policy is normally trained with, both decided on the device inside the
captured rollout (`upkie_amd.events.EpisodeEvents`, one more launch per env step): random pushes on the torso -- each
free env step starts one with probability 0.5 %, 5 to 20 N in a random horizontal direction, held 10 to 30 steps, every env
on a schedule of its own -- and link inertias drawn again (+-20 %) whenever an env's episode ends. The trained policy is
then evaluated twice in an env of its own: pushed harder than in training, and not pushed at all.
EXAMPLE_ENVS shortens the batch as EXAMPLE_STEPS shortens the rollout (smoke tests)."""
import os

import torch
import torch.nn as nn

from _common import steps

import upkie_amd.envs as envs
from upkie_amd.evaluation import evaluate_policy
from upkie_amd.events import EpisodeEvents
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import Ppo
from upkie_amd.utils.robot_state import RobotState
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization


def tower(d_in, d_out):  # SB3 MlpPolicy's default net_arch: [64, 64], tanh
    return nn.Sequential(nn.Linear(d_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, d_out))


def reward(obs, info):  # (a stand-in reward: the reference's is constant)
    return torch.abs(obs[:, 0]).neg_().add_(1.0)


if __name__ == "__main__":
    B, T, iterations = int(os.environ.get("EXAMPLE_ENVS", 4096)), steps(128), 3
    E = min(512, 4 * B)  # evaluation episodes
    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    kw = dict(frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=400)
    make = lambda n, seed: envs.make("Upkie-HIP-Pendulum-Vec", num_envs=n, seed=seed, **kw)  # noqa: E731
    with make(B, 0) as env, make(min(B, 256), 1) as pushed_env, make(min(B, 256), 1) as calm_env:
        events = EpisodeEvents(env, push_prob=0.005, push_norm=(5.0, 20.0), push_steps=(10, 30), inertia_variation=0.2)
        actor, critic = tower(4, 1).to(env.device), tower(4, 1).to(env.device)
        policy = MlpActorCritic.from_modules(actor, critic, nn.Parameter(torch.zeros(1, device=env.device)), action_low=[-1.0], action_high=[1.0])
        model = Ppo(env, policy, n_steps=T, batch_size=B * T // 4, learning_rate=lambda p: 3e-4 * p, target_kl=0.03, reward_fn=reward, events=events)
        model.learn(iterations * T * B)
        for record in model.records:
            print(f"iteration {record['time/iterations']}: " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in record.items()))
        print(f"training: {int(events.pushes.sum())} pushes started, {int(events.episodes.sum())} episodes ended (each with links of its own) "
              f"in {int(events.calls[0])} steps of {B} envs")
        harder = EpisodeEvents(pushed_env, push_prob=0.02, push_norm=(10.0, 30.0), push_steps=(10, 30))
        mean, std = evaluate_policy(policy, pushed_env, n_eval_episodes=E, reward_fn=reward, seed=2, events=harder)
        print(f"evaluate_policy, pushed: {mean:.4g} +/- {std:.4g} over {E} episodes, {int(harder.pushes.sum())} pushes")
        mean, std = evaluate_policy(policy, calm_env, n_eval_episodes=E, reward_fn=reward, seed=2)
        print(f"evaluate_policy, not pushed: {mean:.4g} +/- {std:.4g} over {E} episodes")
