"""Stable-Baselines3's ``PPO(...).learn(...)`` on the device in a dozen lines: `upkie_amd.ppo.Ppo` owns what
ppo_mlp_train_time_limits.py assembles by hand (rollout buffer, VecNormalize, episode statistics, the trainer, the
rollout graph) and adds a linear learning-rate schedule and ``target_kl``, both decided on the device inside the
captured update."""
import torch
import torch.nn as nn

from _common import steps

import upkie_amd.envs as envs
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import Ppo
from upkie_amd.utils.robot_state import RobotState
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization


def tower(d_in, d_out):  # SB3 MlpPolicy's default net_arch: [64, 64], tanh
    return nn.Sequential(nn.Linear(d_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, d_out))


if __name__ == "__main__":
    B, T, iterations = 4096, steps(128), 3
    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=B, frequency=200.0, init_state=init, autoreset_mode="same_step",
                   max_episode_steps=400) as env:
        actor, critic = tower(4, 1).to(env.device), tower(4, 1).to(env.device)
        policy = MlpActorCritic.from_modules(actor, critic, nn.Parameter(torch.zeros(1, device=env.device)), action_low=[-1.0], action_high=[1.0])
        model = Ppo(env, policy, n_steps=T, batch_size=B * T // 4, learning_rate=lambda p: 3e-4 * p, target_kl=0.03,
                    reward_fn=lambda obs, info: torch.abs(obs[:, 0]).neg_().add_(1.0))  # (a stand-in reward: the reference's is constant)
        model.learn(iterations * T * B)
        for record in model.records:
            print(f"iteration {record['time/iterations']}: " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in record.items()))
