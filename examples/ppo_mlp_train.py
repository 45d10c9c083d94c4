"""Full PPO iterations on the device: each is a graphed rollout (policy + env step + VecNormalize, 128 steps replayed as
one graph launch, as in ppo_mlp_normalized_rollout.py), GAE, then Stable-Baselines3's PPO.train as HIP launches
(`upkie_amd.ppo.PpoTrainer`: 10 epochs x 4 minibatches of gradient, clip_grad_norm_ and Adam on the policy's packed
weights). The next rollout reads the trained weights straight from the packed buffer: no re-pack, no host sync."""
import torch
import torch.nn as nn

from _common import steps

import upkie_amd.envs as envs
from upkie_amd.graphs import GraphedLoop
from upkie_amd.normalize import RunningNormalizer
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import STAT_NAMES, PpoTrainer
from upkie_amd.rollout import RolloutBuffer
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
        dev = env.device
        actor, critic = tower(4, 1).to(dev), tower(4, 1).to(dev)
        log_std = nn.Parameter(torch.zeros(1, device=dev))
        policy = MlpActorCritic.from_modules(actor, critic, log_std, action_low=[-1.0], action_high=[1.0], seed=0)
        normalizer = RunningNormalizer.for_env(env, gamma=0.99)
        normalizer.attach(policy)
        trainer = PpoTrainer(policy, n_epochs=10, batch_size=B * T // 4, obs_normalized=True, seed=0)  # (the buffer holds norm_obs)
        buffer = RolloutBuffer(T, B, obs_shape=(4,), action_shape=(1,), device=dev)
        env.reset(seed=0)
        obs = env.observation
        normalizer.reset(obs)
        env_action = torch.empty(B, 1, device=dev)
        stand_in = torch.empty(B, device=dev)
        starts = torch.ones(B, dtype=torch.uint8, device=dev)
        slot = {"t": T - 1}

        def rollout_step():
            t = slot["t"]
            buffer.episode_starts[t].copy_(starts)
            out = policy.act(obs, out={"norm_obs": buffer.observations[t], "action": buffer.actions[t], "value": buffer.values[t],
                                       "log_prob": buffer.log_probs[t], "env_action": env_action})
            next_obs, _, terminated, truncated, _ = env.step(out[0])
            torch.abs(next_obs[:, 0], out=stand_in).neg_().add_(1.0)  # stand-in reward (the reference's is constant, upkie_env.py:230)
            normalizer.step(next_obs, stand_in, terminated, truncated, out={"reward": buffer.rewards[t], "episode_starts": starts})
            slot["t"] = (t + 1) % T

        loop = GraphedLoop(rollout_step, unroll=T, warmup=1)
        for it in range(iterations):
            loop.replay()  # T steps with the current packed weights
            buffer.pos, buffer.full = T, True
            buffer.compute_returns_and_advantage(last_values=policy.value(obs), dones=starts)
            stats = trainer.train(buffer)  # [10, 4, 7] on the device
            last = stats[-1].mean(dim=0).cpu().numpy()
            print(f"iteration {it}: mean normalised reward {float(buffer.rewards.mean()):+.4f}, "
                  + ", ".join(f"{name} {value:+.4g}" for name, value in zip(STAT_NAMES, last)), flush=True)
        print(f"ppo_mlp_train: {iterations} iterations of {T} x {B} steps + {trainer.n_epochs} x {trainer.n_minibatches} minibatch updates, "
              f"log_std {float(log_std):+.4f}")
