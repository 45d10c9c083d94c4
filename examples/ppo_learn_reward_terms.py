"""ppo_learn_pipeline.py with its reward written as terms (`upkie_amd.rewards.RewardTerms`) instead of a Python
callable of torch ops: upright and in place as before (``1 - |pitch| - |position| / 4``), plus what a callable of the
observation alone cannot say: a penalty on the command's rate of change and a fall penalty that a time limit does not
trigger. One launch per rollout step; where an episode ended the reward is that of the terminal observation, not of the
reset one; and every log record carries each term's mean episode sum (``rollout/ep_rew_<name>_mean``), which is what
one watches while tuning the weights."""
import torch
import torch.nn as nn

from _common import steps

import upkie_amd.envs as envs
from upkie_amd.pipeline import AgentPipeline
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import Ppo
from upkie_amd.rewards import RewardTerms, Term, act_rate, obs, one, terminated
from upkie_amd.utils.robot_state import RobotState
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization


def tower(d_in, d_out):  # SB3 MlpPolicy's default net_arch: [64, 64], tanh
    return nn.Sequential(nn.Linear(d_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, d_out))


def terms():  # on the RAW observation (pitch, position, ...) and the command the env received (a ground velocity, m/s)
    return {
        "alive": Term(1.0, taps=[one()]),
        "upright": Term(-1.0, "abs", taps=[obs(0)]),
        "in_place": Term(-0.25, "abs", taps=[obs(1)]),
        "action_rate": Term(-0.01, "square", taps=[act_rate(0)]),  # (m/s^2)^2: the pipeline's lag keeps it small
        "fall": Term(-10.0, taps=[terminated()]),
    }


if __name__ == "__main__":
    B, T, K, iterations = 4096, steps(128), 8, 3
    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=B, frequency=200.0, init_state=init, autoreset_mode="same_step",
                   max_episode_steps=400) as env:
        pipe = AgentPipeline(B, 4, [-1.0], [1.0], dt=1.0 / 200.0, stack=K, integrate_action=True, action_noise=[0.02], action_lag=0.05,
                             observation_noise=[0.002, 0.002, 0.01, 0.01], seed=0, device=env.device)
        reward = RewardTerms(B, 4, 1, dt=1.0 / 200.0, terms=terms(), device=env.device)
        D = pipe.stacked_dim
        actor, critic = tower(D, 1).to(env.device), tower(D, 1).to(env.device)
        # (the policy's output is an acceleration in [-2, 2] m/s^2, integrated by the pipeline into [-1, 1] m/s)
        policy = MlpActorCritic.from_modules(actor, critic, nn.Parameter(torch.zeros(1, device=env.device)), action_low=[-2.0], action_high=[2.0])
        model = Ppo(env, policy, n_steps=T, batch_size=B * T // 4, learning_rate=lambda p: 3e-4 * p, target_kl=0.03, reward=reward,
                    pipeline=pipe)
        model.learn(iterations * T * B)
        for record in model.records:
            print(f"iteration {record['time/iterations']}: " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in record.items()))
