"""Teacher to student across the sim-to-real gap, all on the device (`upkie_amd.distill`): 1. a short `Ppo` run trains a
teacher on the clean pendulum env; 2. `Distillation` fits a student that only ever sees what the robot would -- noised and
lagged frames from an `AgentPipeline`, under the pushes of `EpisodeEvents` -- to the teacher's actions on the clean
observation of the same instant, the teacher driving half of the envs at first and none at the end (DAgger's beta); 3.
`evaluate_policy` of both; 4. the hand-over: two `Ppo` iterations fine-tune the distilled student, under the normaliser it
was fitted under. The sizes are tiny so that it runs in a few seconds; EXAMPLE_ENVS, EXAMPLE_STEPS and EXAMPLE_ITERATIONS
shorten it further (smoke tests)."""
import os

import torch
import torch.nn as nn

from _common import steps

import upkie_amd.envs as envs
from upkie_amd.distill import Distillation
from upkie_amd.evaluation import evaluate_policy
from upkie_amd.events import EpisodeEvents
from upkie_amd.pipeline import AgentPipeline
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import Ppo
from upkie_amd.utils.robot_state import RobotState
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization


def tower(d_in, d_out, width):
    return nn.Sequential(nn.Linear(d_in, width), nn.Tanh(), nn.Linear(width, width), nn.Tanh(), nn.Linear(width, d_out))


def actor_critic(d_in, width, device):
    return MlpActorCritic.from_modules(tower(d_in, 1, width).to(device), tower(d_in, 1, width).to(device), nn.Parameter(torch.zeros(1, device=device)),
                                       action_low=[-1.0], action_high=[1.0])


def reward(obs, info):  # (a stand-in reward: the reference's is constant)
    return torch.abs(obs[:, 0]).neg_().add_(1.0)


def show(what, records):
    for record in records:
        print(f"{what} {record['time/iterations']}: " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in record.items()))


if __name__ == "__main__":
    B, T, iterations = int(os.environ.get("EXAMPLE_ENVS", 1024)), steps(32), int(os.environ.get("EXAMPLE_ITERATIONS", 4))
    E = min(256, B)  # evaluation episodes
    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    kw = dict(frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=400)
    make = lambda n, seed: envs.make("Upkie-HIP-Pendulum-Vec", num_envs=n, seed=seed, **kw)  # noqa: E731
    stages = dict(dt=1.0 / 200.0, stack=4, observation_noise=[0.002, 0.002, 0.01, 0.01], action_lag=0.05)
    with make(B, 0) as clean_env, make(B, 1) as env, make(min(B, 256), 2) as eval_env:
        dev = env.device
        # 1. the teacher: [64, 64] towers on the clean observation
        teacher = actor_critic(4, 64, dev)
        Ppo(clean_env, teacher, n_steps=T, batch_size=B * T // 4, reward_fn=reward).learn(iterations * T * B)
        # 2. the student: [32, 32] towers behind the pipeline, pushed; the teacher reads the raw observation of the same env
        pipeline = AgentPipeline(B, 4, [-1.0], [1.0], seed=3, device=dev, **stages)
        events = EpisodeEvents(env, push_prob=0.005, push_norm=(5.0, 20.0), push_steps=(10, 30))
        student = actor_critic(pipeline.stacked_dim, 32, dev)
        model = Distillation(env, student, teacher, n_steps=T, n_epochs=5, batch_size=B * T // 4, learning_rate=lambda p: 1e-3 * (0.1 + 0.9 * p),
                             beta=lambda p: 0.5 * p, pipeline=pipeline, events=events, reward_fn=reward)
        model.learn(iterations * T * B)
        show("distillation", model.records)
        # 3. both, evaluated where each belongs
        mean, std = evaluate_policy(teacher, eval_env, n_eval_episodes=E, reward_fn=reward, seed=4)
        print(f"teacher on clean observations: {mean:.4g} +/- {std:.4g} over {E} episodes")
        eval_pipeline = AgentPipeline(eval_env.num_envs, 4, [-1.0], [1.0], seed=5, device=dev, **stages)
        mean, std = evaluate_policy(student, eval_env, n_eval_episodes=E, reward_fn=reward, seed=4, pipeline=eval_pipeline)
        print(f"student behind the pipeline: {mean:.4g} +/- {std:.4g} over {E} episodes")
        # 4. the hand-over: the packed weights are the policy, its normaliser stays
        tuned = Ppo(env, student, n_steps=T, batch_size=B * T // 4, reward_fn=reward, pipeline=pipeline, events=events)
        tuned.learn(2 * T * B)
        assert tuned.normalizer is model.normalizer
        show("fine-tune", tuned.records)
