"""The PPO iterations of ppo_mlp_train.py with the two pieces of Stable-Baselines3's collect_rollouts / Monitor that the
rollout still lacked, both inside the one captured rollout graph: the time-limit bootstrap (every env that ended by
max_episode_steps and not by a fall gets reward += gamma * V(final_obs) on its normalised reward, so GAE does not treat
a time limit as a death) and the episode statistics (`upkie_amd.episodes.EpisodeStatistics`: SB3's
rollout/ep_rew_mean and rollout/ep_len_mean over the last 100 episodes, on the raw reward), printed per iteration."""
import math

import torch
import torch.nn as nn

from _common import steps

import upkie_amd.envs as envs
from upkie_amd.episodes import EpisodeStatistics
from upkie_amd.graphs import GraphedLoop
from upkie_amd.normalize import RunningNormalizer
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import STAT_NAMES, PpoTrainer
from upkie_amd.rollout import RolloutBuffer
from upkie_amd.utils.robot_state import RobotState
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization


def tower(d_in, d_out):  # SB3 MlpPolicy's default net_arch: [64, 64], tanh
    return nn.Sequential(nn.Linear(d_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, d_out))


def fmt(x):
    return "n/a" if x is None or math.isnan(x) else f"{x:.4g}"


if __name__ == "__main__":
    B, T, iterations = 4096, steps(128), 3
    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=B, frequency=200.0, init_state=init, autoreset_mode="same_step",
                   max_episode_steps=400) as env:
        dev = env.device
        actor, critic = tower(4, 1).to(dev), tower(4, 1).to(dev)
        log_std = nn.Parameter(torch.zeros(1, device=dev))
        policy = MlpActorCritic.from_modules(actor, critic, log_std, action_low=[-1.0], action_high=[1.0], seed=0)
        normalizer = RunningNormalizer.for_env(env, gamma=0.99)
        normalizer.attach(policy)
        episodes = EpisodeStatistics(B, window=100, device=dev)  # SB3's stats_window_size
        trainer = PpoTrainer(policy, n_epochs=10, batch_size=B * T // 4, obs_normalized=True, seed=0)  # (the buffer holds norm_obs)
        buffer = RolloutBuffer(T, B, obs_shape=(4,), action_shape=(1,), device=dev)
        env.reset(seed=0)
        obs = env.observation
        normalizer.reset(obs)
        env_action = torch.empty(B, 1, device=dev)
        reward = torch.empty(B, device=dev)
        starts = torch.ones(B, dtype=torch.uint8, device=dev)
        slot = {"t": T - 1}

        def rollout_step():
            t = slot["t"]
            buffer.episode_starts[t].copy_(starts)
            out = policy.act(obs, out={"norm_obs": buffer.observations[t], "action": buffer.actions[t], "value": buffer.values[t],
                                       "log_prob": buffer.log_probs[t], "env_action": env_action})
            next_obs, _, terminated, truncated, info = env.step(out[0])
            torch.abs(next_obs[:, 0], out=reward).neg_().add_(1.0)  # stand-in reward (the reference's is constant, upkie_env.py:230)
            episodes.step(reward, terminated, truncated)  # Monitor: the raw reward
            normalizer.step(next_obs, reward, terminated, truncated, out={"reward": buffer.rewards[t], "episode_starts": starts})
            # time limits: bootstrap the normalised reward from the last observation of the envs that truncated
            policy.bootstrap_time_limits(info["final_obs"], terminated, truncated, buffer.rewards[t], buffer.gamma)
            slot["t"] = (t + 1) % T

        loop = GraphedLoop(rollout_step, unroll=T, warmup=1)
        for it in range(iterations):
            loop.replay()  # T steps with the current packed weights
            buffer.pos, buffer.full = T, True
            buffer.compute_returns_and_advantage(last_values=policy.value(obs), dones=starts)
            stats = trainer.train(buffer)  # [10, 4, 7] on the device
            last = stats[-1].mean(dim=0).cpu().numpy()
            print(f"iteration {it}: ep_rew_mean {fmt(episodes.ep_rew_mean())}, ep_len_mean {fmt(episodes.ep_len_mean())}, "
                  f"episodes {episodes.total_episodes}, " + ", ".join(f"{name} {value:+.4g}" for name, value in zip(STAT_NAMES, last)),
                  flush=True)
        print(f"ppo_mlp_train_time_limits: {iterations} iterations of {T} x {B} steps + {trainer.n_epochs} x {trainer.n_minibatches} "
              f"minibatch updates, log_std {float(log_std):+.4f}")
