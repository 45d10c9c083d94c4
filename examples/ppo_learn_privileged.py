"""ppo_learn_events.py with a privileged critic (the asymmetric actor-critic): the actor reads what the robot will see --
the noised observation with the command appended, 8 frames stacked (`upkie_amd.pipeline.AgentPipeline`) --, the critic
what the simulator knows: the raw observation, the command, the push that is acting and the link scales this episode
drew (`upkie_amd.privileged.PrivilegedObservation`, one more launch per env step, `Ppo(critic_observation=...)`). The
critic is not deployed: the trained policy is evaluated as any other, with no privileged row anywhere.
EXAMPLE_ENVS shortens the batch as EXAMPLE_STEPS shortens the rollout (smoke tests)."""
import os

import torch
import torch.nn as nn

from _common import steps

import upkie_amd.envs as envs
from upkie_amd.evaluation import evaluate_policy
from upkie_amd.events import EpisodeEvents
from upkie_amd.pipeline import AgentPipeline
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import Ppo
from upkie_amd.privileged import PrivilegedObservation
from upkie_amd.utils.robot_state import RobotState
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization


def tower(d_in, d_out):  # SB3 MlpPolicy's default net_arch: [64, 64], tanh
    return nn.Sequential(nn.Linear(d_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, d_out))


def reward(obs, info):  # (a stand-in reward: the reference's is constant)
    return torch.abs(obs[:, 0]).neg_().add_(1.0)


def pipeline_for(env):
    return AgentPipeline(env.num_envs, 4, [-1.0], [1.0], dt=1.0 / 200.0, stack=8, observation_noise=[0.01, 0.005, 0.02, 0.02], action_lag=0.05,
                         device=env.device)


if __name__ == "__main__":
    B, T, iterations = int(os.environ.get("EXAMPLE_ENVS", 4096)), steps(128), 3
    E = min(512, 4 * B)  # evaluation episodes
    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    kw = dict(frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=400)
    make = lambda n, seed: envs.make("Upkie-HIP-Pendulum-Vec", num_envs=n, seed=seed, **kw)  # noqa: E731
    with make(B, 0) as env, make(min(B, 256), 1) as eval_env:
        events = EpisodeEvents(env, push_prob=0.005, push_norm=(5.0, 20.0), push_steps=(10, 30), inertia_variation=0.2)
        pipeline = pipeline_for(env)
        rows = PrivilegedObservation(env, events=events, pipeline=pipeline)  # observation, command, push force, link scales
        actor, critic = tower(pipeline.stacked_dim, 1).to(env.device), tower(rows.dim, 1).to(env.device)
        policy = MlpActorCritic.from_modules(actor, critic, nn.Parameter(torch.zeros(1, device=env.device)), action_low=[-1.0], action_high=[1.0])
        print(f"the actor reads {pipeline.stacked_dim} words, the critic {rows.dim}: " + ", ".join(f"{name} {n}" for name, n in zip(rows.include, rows.counts)))
        model = Ppo(env, policy, n_steps=T, batch_size=B * T // 4, learning_rate=lambda p: 3e-4 * p, target_kl=0.03, reward_fn=reward, events=events,
                    pipeline=pipeline, critic_observation=rows)
        model.learn(iterations * T * B)
        for record in model.records:
            print(f"iteration {record['time/iterations']}: " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in record.items()))
        print(f"training: {int(events.pushes.sum())} pushes started, {int(events.episodes.sum())} episodes ended in {int(events.calls[0])} steps of {B} envs")
        harder = EpisodeEvents(eval_env, push_prob=0.02, push_norm=(10.0, 30.0), push_steps=(10, 30))
        mean, std = evaluate_policy(policy, eval_env, n_eval_episodes=E, reward_fn=reward, seed=2, events=harder, pipeline=pipeline_for(eval_env))
        print(f"evaluate_policy, pushed, no critic: {mean:.4g} +/- {std:.4g} over {E} episodes")
