"""ppo_learn.py with the second half of an SB3 training script: `upkie_amd.evaluation.EvalCallback` evaluates the
DETERMINISTIC policy every other iteration in an env of its own (256 envs, another size than the training env's 4096;
the policy's packed statistics keep it in sync with training's VecNormalize), adds ``eval/mean_reward``,
``eval/mean_ep_length`` and ``eval/time_limit_frac`` to that iteration's record and keeps the best mean; then one
`evaluate_policy` of the trained policy, as SB3's. Evaluation is one graph replay per 32 env steps and one host read per
replay, and does not change the training run by a bit."""
import torch
import torch.nn as nn

from _common import steps

import upkie_amd.envs as envs
from upkie_amd.evaluation import EvalCallback, evaluate_policy
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import Ppo
from upkie_amd.utils.robot_state import RobotState
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization


def tower(d_in, d_out):  # SB3 MlpPolicy's default net_arch: [64, 64], tanh
    return nn.Sequential(nn.Linear(d_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, d_out))


def reward(obs, info):  # (a stand-in reward: the reference's is constant)
    return torch.abs(obs[:, 0]).neg_().add_(1.0)


if __name__ == "__main__":
    B, T, iterations = 4096, steps(128), 4
    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    kw = dict(frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=400)
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=B, **kw) as env, envs.make("Upkie-HIP-Pendulum-Vec", num_envs=256, **kw) as eval_env:
        actor, critic = tower(4, 1).to(env.device), tower(4, 1).to(env.device)
        policy = MlpActorCritic.from_modules(actor, critic, nn.Parameter(torch.zeros(1, device=env.device)), action_low=[-1.0], action_high=[1.0])
        model = Ppo(env, policy, n_steps=T, batch_size=B * T // 4, learning_rate=lambda p: 3e-4 * p, target_kl=0.03, reward_fn=reward)
        callback = EvalCallback(eval_env, n_eval_episodes=512, eval_freq=2 * T, reward_fn=reward, seed=1)
        model.learn(iterations * T * B, callback=callback)
        for record in model.records:
            print(f"iteration {record['time/iterations']}: " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in record.items()))
        print(f"best eval/mean_reward {callback.best_mean_reward:.4g} of {len(callback.evaluations['timesteps'])} evaluations at "
              f"{callback.evaluations['timesteps']} timesteps")
        mean, std = evaluate_policy(policy, eval_env, n_eval_episodes=512, reward_fn=reward, seed=2)
        print(f"evaluate_policy: {mean:.4g} +/- {std:.4g} over 512 episodes")
